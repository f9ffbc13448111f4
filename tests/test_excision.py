"""Narrowband interference excision without a GPU: the numpy restatement of the algorithm
(tests/ifx_ref.py, the contract of gpsmi_ifx_*) on the synthetic scene, and the argument errors of
the new C ABI."""
import ctypes as C

import numpy as np
import pytest

import ifx_ref as R

JN_DB, TONE_HZ = 35.0, -2717.3


def _scene(seed=7):
    from gpsmi import synth
    return synth.default_scene(8, seed=seed)


def _tone(sc, b, jn_db=JN_DB, freq=TONE_HZ):
    return R.add_tone(np.zeros(sc.ngps, dtype=np.complex128), jn_db, freq, sc.sample_rate,
                      b * sc.ngps, sc.noise_sigma ** 2)


def test_threshold_off_is_the_identity_across_blocks():
    """Partition of unity, block boundaries (carry) and the flat-window last frame included."""
    sc = _scene()
    ref = R.ExcisionRef(sc.ngps, thresh_db=np.inf)
    for b in range(3):
        x = sc.block_float(b) + _tone(sc, b)
        y, count, mask, _, _ = ref.process(x)
        assert count == 0 and not mask.any()
        assert np.abs(y - x).max() <= 1e-12 * np.sqrt(np.mean(np.abs(x) ** 2))


def test_jammed_scene_loses_the_tone_and_few_bins():
    sc = _scene()
    ref, tone_ref = R.ExcisionRef(sc.ngps), R.ExcisionRef(sc.ngps)
    for b in range(3):
        tone = _tone(sc, b)
        _, count, mask, _, _ = ref.process(sc.block_float(b) + tone)
        left = tone_ref.excise_with(tone, mask)          # (linear for a fixed mask)
        tone_ref.carry = tone[-R.H:].copy()
        if b == 0:
            continue                                     # (block 0 starts behind a zero carry)
        assert 1 <= count <= 40, count
        resid_db = 10 * np.log10(np.vdot(left, left).real / np.vdot(tone, tone).real)
        assert resid_db <= -30.0, resid_db


@pytest.mark.parametrize('seed', [7, 11])
def test_clean_scene_flags_nothing(seed):
    sc = _scene(seed)
    ref = R.ExcisionRef(sc.ngps)
    for b in range(3):
        y, count, mask, P, thr = ref.process(sc.block_float(b))
        assert count == 0 and not mask.any(), (b, count, P.max() / thr)


def test_wideband_interference_passes_through():
    sc = _scene()
    x = sc.block_float(1)
    spec = np.zeros(sc.ngps, dtype=np.complex128)
    spec[4000:20000] = np.exp(2j * np.pi * np.random.default_rng(3).random(16000))
    x = x + np.fft.ifft(spec) * np.sqrt(sc.ngps) * 3.0
    y, count, mask, _, _ = R.ExcisionRef(sc.ngps).process(x)
    assert count == -1 and not mask.any() and np.array_equal(y, x)


def test_dilation_is_circular_and_mask_words_round_trip():
    ref = R.ExcisionRef(8192, dilate=2)
    P = np.ones(R.L)
    P[0] = P[1000] = 100.0
    spectra = np.sqrt(np.stack([P, P, P, P]))
    _, _, mask, count = ref.detect(spectra)
    assert count == 10
    assert sorted(np.flatnonzero(mask)) == [0, 1, 2, 998, 999, 1000, 1001, 1002, 2046, 2047]
    assert np.array_equal(R.words_to_mask(R.mask_words(mask)), mask)
    assert R.mask_words(mask)[0] == 0b111 and R.mask_words(mask)[63] == 0b11 << 30


def _ifx_cfg(n=65536, thresh=6.0, dilate=2, max_bins=256):
    from gpsmi import _lib
    return _lib.IfxCfg(n, thresh, dilate, max_bins, 0)


def test_abi_argument_errors_do_not_need_a_gpu():
    from gpsmi import _lib
    lib = _lib.load()
    h = C.c_void_p(0xDEAD)
    assert lib.gpsmi_ifx_create(None, C.byref(h)) == -1                     # GPSMI_E_ARG
    assert lib.gpsmi_ifx_create(C.byref(_ifx_cfg()), None) == -1
    for bad in (_ifx_cfg(thresh=float('nan')), _ifx_cfg(dilate=-1), _ifx_cfg(dilate=65),
                _ifx_cfg(max_bins=-1), _ifx_cfg(max_bins=2049)):
        h = C.c_void_p(0xDEAD)
        assert lib.gpsmi_ifx_create(C.byref(bad), C.byref(h)) == -1 and h.value is None
    for n in (16368 * 8, 16368 * 32, 65536 + 512, 3072, 0, -1024):           # GPSMI_E_UNSUPPORTED
        h = C.c_void_p(0xDEAD)
        assert lib.gpsmi_ifx_create(C.byref(_ifx_cfg(n)), C.byref(h)) == -5 and h.value is None
        assert b'block_samples' in lib.gpsmi_last_error()
    buf = np.zeros(16, dtype=np.complex64)
    assert lib.gpsmi_ifx_apply(None, _lib.ptr(buf), _lib.ptr(buf), 1, None, None) == -1
    assert lib.gpsmi_ifx_apply_dev(None, 1, 2, 1, None, None) == -1
    assert lib.gpsmi_ifx_set_input_format(None, 0) == -1
    assert lib.gpsmi_ifx_reset(None) == -1
    assert lib.gpsmi_ifx_last_ms(None, None) == -1
    assert lib.gpsmi_ifx_last_psd(None, None) == -1
    assert lib.gpsmi_ifx_destroy(None) == 0


def test_unsupported_config_raises_engine_error():
    from gpsmi.engine import Config, EngineError
    from gpsmi.excision import Excision
    with pytest.raises(EngineError, match=r'\(-5\)'):
        Excision(Config(code_samples=16368, n_cyc=8))
