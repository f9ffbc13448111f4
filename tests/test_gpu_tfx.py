"""Time-frequency (sweep) excision on the GPU (gpsmi_tfx_*, csrc/gpsmi_tfx.hip): what does not change
a bit (the cut of the input into calls, the input format, the entry point, a block that passes
through) and what the stage buys: acquisition and tracking through a swept jammer at 2.048 Msps and
through the +-8 MHz / 20 us chirp at 16.368 Msps, alone and in the chain of a receiver."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import ifx_ref
import pb_ref
import tfx_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_DB = 30.0
ROWS = {2048: (0.8e6, 1e-3), 16368: (8e6, 20e-6)}          # span, period of the jammer per code length
U8_SCALE = 0.08                 # the sweep's amplitude 0.89 of the 8-bit range: no component clips
_CACHE = {}


def _scene(code_samples=2048, n_cyc=32):
    from gpsmi import synth
    key = ('scene', code_samples)
    if key not in _CACHE:
        _CACHE[key] = synth.default_scene(8, seed=7, code_samples=code_samples, n_cyc=n_cyc)
    return _CACHE[key]


def _swept(b, sc=None, extra=False):
    """complex128 block b of the scene under the sweep; extra: a CW tone and 20 dB pulses as well."""
    sc = sc or _scene()
    key = ('swept', sc.code_samples, b, extra)
    if key not in _CACHE:
        n, np_ = sc.ngps, sc.noise_sigma ** 2
        span, period = ROWS[sc.code_samples]
        x = sc.block_float(b) + R.sweep(b * n, n, sc.sample_rate, SWEEP_DB, np_, span, period)
        if extra:
            x = pb_ref.add_pulses(x, np_, seed=1000 + b, jn_db=20.0, width=8)[0]
            x = ifx_ref.add_tone(x, 35.0, -2717.3, sc.sample_rate, b * n, np_)
        _CACHE[key] = x
    return _CACHE[key]


def _c64(blocks):
    return np.stack([np.asarray(x, dtype=np.complex64) for x in blocks])


def _results(sx):
    return sx.last_counts.copy(), sx.last_floors.copy(), sx.last_masks.copy()


def _same_results(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize('L', R.FRAMES)
def test_the_cut_into_calls_and_the_entry_point_do_not_change_a_bit(L):
    from gpsmi.engine import Config, DeviceBuffer
    from gpsmi.tfexcision import SweepExcision
    n = 4096
    xs = _c64((R.noise(40 + L, 4 * n) + R.sweep(0, 4 * n, 2.048e6, 30.0, R.NOISE_POWER, 0.8e6, 1e-3)).reshape(4, n))
    d_in, d_out = DeviceBuffer(xs.nbytes), DeviceBuffer(xs.nbytes)
    d_in.upload(xs)
    sx = SweepExcision(Config(code_samples=1024, n_cyc=4), frame=L)
    sx.apply_dev(d_in.ptr, d_out.ptr, 4)
    batched, res = d_out.download(np.complex64, 4 * n), _results(sx)
    assert (res[0] > 0).all()
    for cut in ([1, 3], [1, 1, 1, 1]):
        sx.reset()
        b0 = 0
        for k in cut:
            sx.apply_dev(d_in.at(b0 * n * 8), d_out.at(b0 * n * 8), k)
            assert _same_results(_results(sx), tuple(r[b0:b0 + k] for r in res)), (cut, b0)
            b0 += k
        assert d_out.download(np.complex64, 4 * n).tobytes() == batched.tobytes(), cut
    sx.reset()
    assert sx.apply(xs).tobytes() == batched.tobytes()           # apply == apply_dev
    assert _same_results(_results(sx), res)
    sx.reset()
    sx.apply_dev(d_in.ptr, d_out.ptr, 1)                         # reset restores the first result
    assert d_out.download(np.complex64, n).tobytes() == batched[:n].tobytes()
    from gpsmi._lib import EngineError
    with pytest.raises(EngineError, match='overlap'):
        sx.apply_dev(d_in.ptr, d_in.ptr, 1)
    sx.close()
    d_in.free()
    d_out.free()


def test_large_call_grid_equals_single_calls():
    """40 blocks of 16384 in one call (the long runs of frames per workgroup) against 40 single calls."""
    from gpsmi.engine import Config
    from gpsmi.tfexcision import SweepExcision
    n, nb = 16384, 40
    xs = _c64((R.noise(77, nb * n) + R.sweep(0, nb * n, 2.048e6, 30.0, R.NOISE_POWER, 0.8e6, 1e-3)).reshape(nb, n))
    cfg = Config(code_samples=1024, n_cyc=16)
    for L in (32, 256):
        a, b = SweepExcision(cfg, frame=L), SweepExcision(cfg, frame=L)
        y = a.apply(xs)
        singles = np.stack([b.apply(x) for x in xs])
        assert y.tobytes() == singles.tobytes() and (a.last_counts > 0).all()
        a.close()
        b.close()


def test_u8_input_equals_complex64_of_the_decode_and_a_format_switch_keeps_the_carry():
    from gpsmi import synth
    from gpsmi._lib import check
    from gpsmi.engine import Config
    from gpsmi.tfexcision import SweepExcision
    n = 4096
    cfg = Config(code_samples=1024, n_cyc=4)
    x = (R.noise(50, 3 * n) + R.sweep(0, 3 * n, 2.048e6, 30.0, R.NOISE_POWER, 0.8e6, 1e-3)).reshape(3, n) * U8_SCALE
    raw = R.quantise(x)
    dec = synth.raw_to_c64(raw)
    s_u8, s_c = SweepExcision(cfg, raw_u8=True), SweepExcision(cfg)
    y_u8, y_c = s_u8.apply(raw), s_c.apply(dec)
    assert (s_u8.last_counts > 0).all()
    assert _same_results(_results(s_u8), _results(s_c)) and y_u8.tobytes() == y_c.tobytes()
    s_u8.close()
    for first_u8 in (False, True):
        s_c.reset()
        got = []
        for b, u8 in enumerate((first_u8, not first_u8, first_u8)):
            check(s_c.lib.gpsmi_tfx_set_input_format(s_c.h, int(u8)), 'gpsmi_tfx_set_input_format')
            s_c.raw_u8 = u8
            got.append(s_c.apply(raw[b] if u8 else dec[b]))
        assert np.stack(got).tobytes() == y_c.tobytes()
    s_c.close()


def test_a_block_that_passes_through_leaves_its_neighbours_as_computed():
    """Tones on every seventh bin of every frame, far above a low floor: 27 of 64 cells detected (the
    median stays on the floor), 45 of 64 flagged once widened: over max_frac = 0.5."""
    from gpsmi.engine import Config
    from gpsmi.tfexcision import SweepExcision
    n, L = 4096, 64
    cfg = Config(code_samples=1024, n_cyc=4)
    xs = (R.noise(60, 3 * n) + R.sweep(0, 3 * n, 2.048e6, 30.0, R.NOISE_POWER, 0.8e6, 1e-3)).reshape(3, n)
    xs[1] = R.comb(n, L, 7) + 1e-3 * R.noise(61, n)
    xs = _c64(xs)
    sx = SweepExcision(cfg, keep_power=True)
    y = sx.apply(xs)
    res, power = _results(sx), sx.last_power()
    assert res[0][1] == -1 and res[0][0] > 0 and res[0][2] > 0
    assert y[1].tobytes() == xs[1].tobytes() and not res[2][1].any()
    for b in range(3):                                          # floors, masks, counts from the kept P
        f32, m32, c32 = R.detect_from_power(power[b])
        assert res[1][b] == f32 and res[0][b] == c32 and np.array_equal(R.words_to_mask(res[2][b], L), m32)
    # the float64 restatement: the same classes, block 2 behind the comb's tail as its carry
    ref = R.SweepRef(n, L)
    y_r, c_r, m_r, _ = ref.run(xs)
    assert c_r[1] == -1 and np.array_equal(R.words_to_mask(res[2][2], L), m_r[2])
    assert np.abs(y[2] - y_r[2]).max() <= 1e-5 * R.rms(xs[2])   # (float32 against float64: coarse on purpose,
    # the bound proper is tests/test_gpu_tfx_ref.py's; a carry from anywhere else is off by the jammer's level)
    one = SweepExcision(cfg)
    singles = np.stack([one.apply(x) for x in xs])
    assert singles.tobytes() == y.tobytes()
    one.close()
    # raw u8: the block passes through as the bytes of its decode
    raw = R.quantise(xs.astype(np.complex128) * U8_SCALE)
    s8 = SweepExcision(cfg, raw_u8=True)
    y8 = s8.apply(raw)
    assert s8.last_counts[1] == -1 and y8[1].tobytes() == R.raw_to_c64(raw[1]).tobytes()
    s8.close()
    sx.close()


def test_all_zero_block_and_threshold_off():
    from gpsmi.engine import Config
    from gpsmi.tfexcision import SweepExcision
    n = 4096
    cfg = Config(code_samples=1024, n_cyc=4)
    xs = _c64((R.noise(70, 2 * n) + R.sweep(0, 2 * n, 2.048e6, 30.0, R.NOISE_POWER, 0.8e6, 1e-3)).reshape(2, n))
    zero = np.zeros((1, n), dtype=np.complex64)
    for L in R.FRAMES:
        sx = SweepExcision(cfg, frame=L)
        y = sx.apply(np.concatenate([zero, zero, xs]))
        assert sx.last_counts[:2].tolist() == [0, 0] and not y[:2].any() and not sx.last_floors[:2].any()
        assert (sx.last_counts[2:] > 0).all()
        sx.close()
        off = SweepExcision(cfg, frame=L, thresh_db=float('inf'))
        y = off.apply(xs)
        assert (off.last_counts == 0).all() and not off.last_masks.any()
        assert np.abs(y - xs).max() <= 4e-6 * R.rms(xs)         # (two float32 transforms of 11 dB peak-to-RMS)
        off.close()


def _nm_table(eng, x, prns, freqs):
    t = eng.search(x, prns, freqs, 4)
    return (t['peak'].astype(np.float64) - t['mean']) / t['std'], t['argmax']


def test_acquisition_through_the_sweep():
    """Fails without the stage: +-0.8 MHz per 1 ms, 30 dB up, buries the satellites below CORR_MIN."""
    from gpsmi.engine import AcqEngine, Config
    from gpsmi.tfexcision import SweepExcision
    cfg = Config()
    sc = _scene()
    prns = [s.prn for s in sc.sats]
    freqs = [cfg.min_freq + cfg.step_freq * i for i in range(50)]
    jam = _c64([_swept(b) for b in (0, 1)])
    clean = np.asarray(sc.block_float(1), dtype=np.complex64)
    sx = SweepExcision()
    out = sx.apply(jam)[1]
    share = sx.last_counts[1] / (2 * sc.ngps)
    sx.close()
    assert 0.05 < share < 0.3, share
    eng = AcqEngine(cfg)
    nm_c, am_c = _nm_table(eng, clean, prns, freqs)
    nm_j, _ = _nm_table(eng, jam[1], prns, freqs)
    nm_x, am_x = _nm_table(eng, out, prns, freqs)
    eng.close()
    print('share', share, 'nMC clean', nm_c.max(axis=0).round(1), 'jammed', nm_j.max(axis=0).round(1),
          'excised', nm_x.max(axis=0).round(1))
    col = np.arange(len(prns))
    assert (nm_c.max(axis=0) > cfg.corr_min).all()
    assert (nm_j.max(axis=0) > cfg.corr_min).sum() <= 1, nm_j.max(axis=0)
    assert (nm_x.max(axis=0) > cfg.corr_min).all(), nm_x.max(axis=0)
    best_c, best_x = nm_c.argmax(axis=0), nm_x.argmax(axis=0)
    assert np.array_equal(best_x, best_c), (best_x, best_c)
    d = np.abs(am_x[best_x, col].astype(np.int64) - am_c[best_x, col])
    assert (np.minimum(d, cfg.code_samples - d) <= 1).all()


def test_acquisition_at_16368_through_the_chirp():
    """+-8 MHz per 20 us inside the 16 MHz band: the tone excision refuses this rate and the blanker sees
    a constant envelope; frames of 32 samples."""
    from gpsmi.acquisition import Acquisition
    from gpsmi.engine import Config
    from gpsmi.tfexcision import SweepExcision
    cfg = Config(code_samples=16368, n_cyc=8)
    sc = _scene(16368, 8)
    xs = _c64([_swept(b, sc) for b in (0, 1)])
    sx = SweepExcision(cfg)
    assert sx.frame == 32
    out = sx.apply(xs)[1]
    share = sx.last_counts[1] / (2 * sc.ngps)
    sx.close()
    assert 0.1 < share < 0.45, share
    prns = [s.prn for s in sc.sats]
    freqs = [cfg.min_freq + cfg.step_freq * i for i in range(50)]
    acq = Acquisition(cfg)
    t_j = acq.search_table(xs[1], prns, freqs, 4)
    t = acq.search_table(out, prns, freqs, 4)
    acq.engine.close()
    nm_j = (t_j['peak'].astype(np.float64) - t_j['mean']) / t_j['std']
    nm = (t['peak'].astype(np.float64) - t['mean']) / t['std']
    print('share', share, 'nMC jammed', nm_j.max(axis=0).round(1), 'excised', nm.max(axis=0).round(1))
    assert (nm_j.max(axis=0) > cfg.corr_min).sum() <= 1, nm_j.max(axis=0)
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


def test_receiver_with_sweep_equals_receiver_on_excised_blocks():
    from gpsmi.pipeline import Receiver
    from gpsmi.tfexcision import SweepExcision
    xs = _c64([_swept(b) for b in range(64)])
    sx = SweepExcision()
    cleaned = sx.apply(xs)
    assert (sx.last_counts > 0).all()
    sx.close()
    _run_pair(Receiver(sweep=True), Receiver(), xs, cleaned)


def test_receiver_raw_u8_with_sweep():
    from gpsmi.pipeline import Receiver
    from gpsmi.tfexcision import SweepExcision
    scaled = [_swept(b) * U8_SCALE for b in range(64)]
    clip = np.mean([np.mean(np.abs(np.concatenate([x.real, x.imag])) > 1.0) for x in scaled[:4]])
    assert clip < 0.01, clip
    raw = np.stack([R.quantise(x) for x in scaled])
    sx = SweepExcision(raw_u8=True)
    cleaned = sx.apply(raw)
    assert (sx.last_counts > 0).all()
    sx.close()
    _run_pair(Receiver(raw_u8=True, sweep=True), Receiver(), raw, cleaned)
    with pytest.raises(ValueError, match='SweepExcision'):
        Receiver(raw_u8=True, sweep=SweepExcision())


def test_receiver_chain_equals_the_three_stages_one_after_another():
    """A tone 35 dB up, the sweep 30 dB up and pulses 20 dB up: excision, sweep excision, blanking, in
    that order on the device, byte for byte what the three handles give one after another."""
    from gpsmi.blanking import PulseBlanker
    from gpsmi.excision import Excision
    from gpsmi.pipeline import Receiver
    from gpsmi.tfexcision import SweepExcision
    xs = _c64([_swept(b, extra=True) for b in range(8)])
    ex, sx, pb = Excision(), SweepExcision(), PulseBlanker()
    cleaned = pb.apply(sx.apply(ex.apply(xs)))
    assert (ex.last_counts > 0).all() and (sx.last_counts > 0).all() and (pb.last_counts > 0).all()
    for s in (ex, sx, pb):
        s.close()
    rx_a, rx_b = Receiver(excise=True, sweep=True, blank=True), Receiver()
    assert rx_a.conditioner.stages == [rx_a.excision, rx_a.sweeper, rx_a.blanker]
    for a, b in zip(xs, cleaned):
        assert rx_a.feed(a) == rx_b.feed(np.ascontiguousarray(b))
        assert np.asarray(rx_a.conditioner.last).tobytes() == b.tobytes()
    assert rx_a.found_sats == rx_b.found_sats
    rx_a.close()
    rx_b.close()


def test_run_file_sweep_on_a_raw_recording(tmp_path):
    """tools/run_file.py --sweep: raw uint16 in, the stage decodes, the engines run on its output."""
    sc = _scene()
    path = str(tmp_path / 'swept.bin')
    with open(path, 'wb') as f:
        for b in range(40):
            R.quantise(_swept(b) * U8_SCALE).astype('<u2').tofile(f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), path, '--sweep', '--json'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['blocks'] == 40 and out['datagrams'] >= 1
    assert out['sweep']['frame'] == 64 and out['sweep']['blocks_excised'] == 40
    assert 0.05 < out['sweep']['mean_share'] < 0.3
    assert {s for s, _, _ in out['acquired']} == {s.prn for s in sc.sats}
    assert sorted(out['tracked']) == sorted(s.prn for s in sc.sats)


def test_run_file_sweep_reaches_a_position_fix(tmp_path):
    """tools/run_file.py --sweep on 22 s of the geometric scene of tests/test_run_file.py under the sweep,
    in the recorder's 8 bits, ephemerides supplied: the stage is reported and the fix lies within 5 m of
    the truth (the bar of test_recording_to_position_fix for the clean scene)."""
    from gpsmi import position as P, synth_nav
    seconds = 22.0
    truth = np.array(P.geo_to_ecef(49.082961, 8.307581, 160.0))
    sc, info = synth_nav.geometric_scene(truth, seconds)
    n, n_blocks = sc.ngps, int(seconds / 0.032)
    span, period = ROWS[sc.code_samples]
    path = str(tmp_path / 'swept_nav.bin')
    with open(path, 'wb') as f:
        for b in range(n_blocks):
            x = sc.block_float(b) + R.sweep(b * n, n, sc.sample_rate, SWEEP_DB, sc.noise_sigma ** 2, span, period)
            R.quantise(x * U8_SCALE).astype('<u2').tofile(f)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), path, '--ephemeris', eph,
                        '--sweep', '--json'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print({k: out[k] for k in ('blocks', 'datagrams', 'fixes', 'tracked', 'sweep')}, out.get('position'))
    assert out['blocks'] == n_blocks and len(out['tracked']) >= 6
    assert out['sweep']['frame'] == 64 and out['sweep']['blocks_excised'] == n_blocks
    assert out['sweep']['blocks_passed_through'] == 0
    assert out['fixes'] > 150
    pos = np.array(out['position']['ecef_m'])
    assert np.linalg.norm(pos - truth) < 5.0, np.linalg.norm(pos - truth)
