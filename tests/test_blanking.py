"""Pulse blanking without a GPU: the numpy restatement of the contract (tests/pb_ref.py, what
gpsmi_pb_* must equal bit for bit) on the synthetic scenes, and the argument errors of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import pb_ref as R


def _scene(seed=7, **kw):
    from gpsmi import synth
    return synth.default_scene(8, seed=seed, **kw)


def _c64(x):
    return np.asarray(x, dtype=np.complex64)


def test_threshold_off_is_the_identity_across_blocks():
    sc = _scene()
    ref = R.BlankerRef(sc.ngps, thresh_db=np.inf)
    for b in range(3):
        x, _ = R.add_pulses(sc.block_float(b), sc.noise_sigma ** 2, seed=b)
        x = _c64(x)
        y, count, m, blank = ref.process(x)
        assert count == 0 and not blank.any() and m > 0
        assert y.tobytes() == x.tobytes()
        assert ref.carry == 0


def test_clean_detection_rate_is_near_two_to_the_minus_f():
    """Complex Gaussian noise exceeds f times its median with probability 2^-f (the exponential
    distribution's median is ln 2 times its mean)."""
    sc = _scene()
    ref = R.BlankerRef(sc.ngps, pre=0, post=0)
    f = float(ref.f)
    rates = []
    for b in range(3):
        _, count, _, _ = ref.process(_c64(sc.block_float(b)))
        rates.append(count / sc.ngps)
    rate = float(np.mean(rates))
    assert 0.5 * 2.0 ** -f <= rate <= 2.0 * 2.0 ** -f, (rate, 2.0 ** -f)


def test_every_burst_sample_above_threshold_is_blanked():
    sc = _scene()
    ref = R.BlankerRef(sc.ngps)
    x, on = R.add_pulses(sc.block_float(1), sc.noise_sigma ** 2, seed=3)
    x = _c64(x)
    y, count, m, blank = ref.process(x)
    p = R.power(x)
    T = np.float32(m * ref.f)
    above = p > T
    assert above[on].mean() > 0.95                 # (the bursts are 30 dB up)
    assert blank[above].all() and (y[blank] == 0).all()
    assert y[~blank].tobytes() == x[~blank].tobytes()
    assert 0 < count <= ref.limit
    # the median stays on the noise at 15 % duty: it moves to the noise's 0.5 / 0.85 quantile, 1.28
    # times the clean median for exponential powers (the mean would move 150-fold)
    m_clean = R.lower_median(R.power(_c64(sc.block_float(1))))
    assert 1.1 < float(m) / float(m_clean) < 1.45


def _spike_block(n, idx, level=100.0):
    x = np.full(n, 0.1 + 0.1j, dtype=np.complex64)
    x[idx] = level
    return x


def test_carry_reaches_exactly_post_samples_into_the_next_block():
    n, pre, post = 2048, 3, 5
    ref = R.BlankerRef(n, pre=pre, post=post)
    y, count, _, blank = ref.process(_spike_block(n, n - 1))
    assert count == pre + 1 and np.flatnonzero(blank).tolist() == list(range(n - 1 - pre, n))
    assert ref.carry == post
    y, count, _, blank = ref.process(_spike_block(n, []))
    assert np.flatnonzero(blank).tolist() == list(range(post)) and count == post
    assert ref.carry == 0
    # a detection at 0 reaches nothing before it, only post after it
    ref.reset()
    _, count, _, blank = ref.process(_spike_block(n, 0))
    assert np.flatnonzero(blank).tolist() == list(range(post + 1))
    # reset clears the carry
    ref.process(_spike_block(n, n - 1))
    ref.reset()
    _, count, _, blank = ref.process(_spike_block(n, []))
    assert count == 0 and not blank.any()


def test_over_max_frac_passes_through():
    n = 4096
    ref = R.BlankerRef(n, pre=0, post=2, max_frac=0.25)
    x = _spike_block(n, np.arange(0, n, 3))          # a third of the samples, every third
    y, count, m, blank = ref.process(x)
    assert count == -1 and not blank.any() and y.tobytes() == x.tobytes()
    assert m == np.float32(0.1) * np.float32(0.1) + np.float32(0.1) * np.float32(0.1)
    assert ref.carry == 2                              # (n - 1 is a detection: still carried)


def test_all_zero_and_constant_blocks_blank_nothing():
    n = 4096
    ref = R.BlankerRef(n)
    for x in (np.zeros(n, dtype=np.complex64), np.full(n, 0.3 - 0.7j, dtype=np.complex64)):
        y, count, m, blank = ref.process(x)
        assert count == 0 and not blank.any() and y.tobytes() == x.tobytes()
    y, count, m, _ = R.BlankerRef(n, thresh_db=np.inf).process(np.zeros(n, dtype=np.complex64))
    assert count == 0 and m == 0


def test_floor_is_the_lower_median_of_tied_powers():
    sc = _scene()
    from gpsmi import synth
    x = synth.raw_to_c64(sc.block_raw(2))               # (the recorder's 8 bits: many ties)
    p = R.power(x)
    m = R.lower_median(p)
    assert m == np.sort(p)[(len(p) - 1) // 2]
    assert (p == m).sum() > 1
    assert (p < m).sum() <= (len(p) - 1) // 2 < (p <= m).sum()


def test_mask_words_round_trip():
    rng = np.random.default_rng(1)
    b = rng.random(4096) < 0.1
    w = R.mask_words(b)
    assert w.dtype == np.uint32 and w.shape == (128,)
    assert np.array_equal(R.words_to_mask(w), b)
    b2 = np.zeros(64, dtype=bool)
    b2[[0, 33, 63]] = True
    assert R.mask_words(b2).tolist() == [1, (1 << 1) | (1 << 31)]


def test_default_guard():
    from gpsmi.blanking import default_guard
    assert default_guard(2048) == 2 and default_guard(16368) == 16 and default_guard(4096) == 4


def _pb_cfg(n=65536, thresh=10.0, pre=2, post=2, max_frac=0.5):
    from gpsmi import _lib
    return _lib.PbCfg(n, thresh, pre, post, max_frac, 0)


def test_abi_argument_errors_do_not_need_a_gpu():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(6) == C.sizeof(_lib.PbCfg) == 24
    h = C.c_void_p(0xDEAD)
    assert lib.gpsmi_pb_create(None, C.byref(h)) == -1                      # GPSMI_E_ARG
    assert lib.gpsmi_pb_create(C.byref(_pb_cfg()), None) == -1
    bad = [_pb_cfg(thresh=float('nan')), _pb_cfg(pre=-1), _pb_cfg(pre=1025), _pb_cfg(post=-1),
           _pb_cfg(post=1025), _pb_cfg(max_frac=-0.1), _pb_cfg(max_frac=1.5), _pb_cfg(max_frac=float('nan'))]
    bad += [_pb_cfg(n) for n in (0, -32, 1024, 2047, 2048 + 16, 65536 + 1, (1 << 24) + 32)]
    for cfg in bad:
        h = C.c_void_p(0xDEAD)
        assert lib.gpsmi_pb_create(C.byref(cfg), C.byref(h)) == -1 and h.value is None
    buf = np.zeros(16, dtype=np.complex64)
    assert lib.gpsmi_pb_apply(None, _lib.ptr(buf), _lib.ptr(buf), 1, None, None, None) == -1
    assert lib.gpsmi_pb_apply_dev(None, 16, 32, 1, None, None, None) == -1
    assert lib.gpsmi_pb_set_input_format(None, 0) == -1
    assert lib.gpsmi_pb_reset(None) == -1
    assert lib.gpsmi_pb_last_ms(None, None) == -1
    assert lib.gpsmi_pb_destroy(None) == 0


def test_python_wrapper_rejects_bad_arguments_without_a_gpu():
    from gpsmi.engine import Config, EngineError
    from gpsmi.blanking import PulseBlanker
    with pytest.raises(EngineError, match=r'\(-1\)'):
        PulseBlanker(Config(), pre=2000)
    with pytest.raises(EngineError, match=r'\(-1\)'):
        PulseBlanker(Config(), max_frac=2.0)
