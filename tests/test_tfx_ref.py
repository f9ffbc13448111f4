"""Time-frequency (sweep) excision without a GPU: the float64 restatement of the contract
(tests/tfx_ref.py, what gpsmi_tfx_* is held to) on the synthetic scenes, the float32 oracle's own
distance from it on the GPU tests' case table, and the argument errors of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import gps_oracle as orc
import tfx_ref as R

_CACHE = {}


def _scene(code_samples=2048, n_cyc=32):
    from gpsmi import synth
    key = ('scene', code_samples)
    if key not in _CACHE:
        _CACHE[key] = synth.default_scene(8, seed=7, code_samples=code_samples, n_cyc=n_cyc)
    return _CACHE[key]


def _nmc(x, sc):
    """normMaxCorr per satellite: the 4-ms search over 51 bins, the maximum over the bins."""
    p = orc.Params(code_samples=sc.code_samples, n_cyc=sc.n_cyc)
    freqs = [p.min_freq + p.step_freq * i for i in range(51)]
    key = ('spectra', sc.code_samples)
    if key not in _CACHE:
        _CACHE[key] = {s.prn: orc.fft_cacode(s.prn, sc.code_samples) for s in sc.sats}
    t = orc.acq_table(np.asarray(x, dtype=np.complex64), freqs, [s.prn for s in sc.sats], 4, p,
                      spectra=_CACHE[key])
    return ((t['peak'] - t['mean']) / t['std']).max(axis=0)


def test_threshold_off_is_the_identity_across_blocks():
    """+inf flags nothing: the windows sum to one over the carry, the Hann frames and the flat half of
    the last frame, at every frame length."""
    n = 4096
    for L in R.FRAMES:
        ref = R.SweepRef(n, L, thresh_db=np.inf)
        x = R.noise(11, 3 * n) + R.sweep(0, 3 * n, 2.048e6, 30.0, R.NOISE_POWER, 0.8e6, 1e-3)
        x = x.reshape(3, n)
        for b in range(3):
            y, count, mask, P, floor, T = ref.process(x[b])
            assert count == 0 and not mask.any() and floor > 0
            assert np.abs(y - x[b]).max() <= 1e-12 * R.rms(x[b])
            assert np.array_equal(ref.carry, x[b, -L // 2:])


def test_last_frame_window_carries_eleven_sixths_of_hann():
    """(3/16 + 1/2) / (3/8) of the continuous window; the sampled one has half a sample less in its
    flat half's favour: 4 / (3 L) below.  The contract's factor is 11/6 at every L."""
    for L in R.FRAMES:
        w = R.window(L)
        wl = w.copy()
        wl[L // 2:] = 1.0
        assert abs((wl ** 2).sum() / (w ** 2).sum() - (R.LAST_GAIN - 4.0 / (3 * L))) < 1e-12


def test_clean_scene_loses_nothing():
    """12 dB on a clean block: under 0.1 % of the cells (complex Gaussian noise exceeds f times its
    median with probability 2^-f: 0.0017 % at 15.8), every satellite found as before."""
    sc = _scene()
    ref = R.SweepRef(sc.ngps, 64)
    ref.process(sc.block_float(0))
    x = sc.block_float(1)
    y, count, mask, *_ = ref.process(x)
    share = count / mask.size
    print('clean: share', share, 'nMC', _nmc(x, sc).round(1), '->', _nmc(y, sc).round(1))
    assert 0 <= share < 1e-3
    assert (_nmc(y, sc) > 8).all()


@pytest.mark.parametrize('row', ['2048-1ms-30dB-L64', '16368-20us-30dB-L32'])
def test_swept_scenes(row):
    """The two swept scenes of DESIGN.md 4.2m's table: none of 8 found through the sweep, all 8 behind
    the filter (block 1 behind block 0)."""
    cs, n_cyc, span, period, L = (2048, 32, 0.8e6, 1e-3, 64) if row.startswith('2048') else (16368, 8, 8e6, 20e-6, 32)
    sc = _scene(cs, n_cyc)
    n, fs = sc.ngps, sc.sample_rate
    ref = R.SweepRef(n, L)
    jam = [sc.block_float(b) + R.sweep(b * n, n, fs, 30.0, sc.noise_sigma ** 2, span, period) for b in (0, 1)]
    ref.process(jam[0])
    y, count, mask, *_ = ref.process(jam[1])
    before, after = _nmc(jam[1], sc), _nmc(y, sc)
    out_db = 10 * np.log10(R.rms(y) ** 2 / R.rms(jam[1]) ** 2)
    print(row, 'share', count / mask.size, 'before', before.round(1), 'after', after.round(1), 'out dB', out_db)
    assert count > 0
    assert (before <= 8).all(), before
    assert (after > 8).all(), after


def test_comb_passes_through():
    """Tones on every third bin: under the Hann window each fills its bin and leaves a quarter of its
    power in either neighbour, so the median sits 6 dB below the tones.  At 3 dB a third of every frame
    is detected, widened by one bin that is the whole plane: over max_frac."""
    n, L = 4096, 64
    x = R.comb(n, L).astype(np.complex64)
    x = x + (1e-3 * R.noise(5, n)).astype(np.complex64)
    ref = R.SweepRef(n, L, thresh_db=3.0)
    y, count, mask, *_ = ref.process(x)
    assert count == -1 and not mask.any()
    assert y.astype(np.complex64).tobytes() == x.tobytes()
    assert np.array_equal(ref.carry, x[-L // 2:].astype(np.complex128))


def test_all_zero_block():
    n = 2048
    for L in R.FRAMES:
        ref = R.SweepRef(n, L)
        y, count, mask, P, floor, T = ref.process(np.zeros(n, dtype=np.complex64))
        assert count == 0 and not mask.any() and floor == 0 and not y.any()
        f, m, c = R.detect_from_power(np.zeros((ref.nf, L), dtype=np.float32))
        assert c == 0 and not m.any() and f == 0


def test_widening_is_circular_and_masks_round_trip():
    L, nf = 64, 6
    raw = np.zeros((nf, L), dtype=bool)
    raw[0, 0] = raw[1, L - 1] = raw[2, 31] = raw[3, 32] = True
    m = R.widen(raw, 2)
    assert np.flatnonzero(m[0]).tolist() == [0, 1, 2, 62, 63]
    assert np.flatnonzero(m[1]).tolist() == [0, 1, 61, 62, 63]
    assert np.flatnonzero(m[2]).tolist() == [29, 30, 31, 32, 33]
    assert not m[4].any() and not m[5].any()                   # (none in time)
    w = R.mask_words(m)
    assert w.dtype == np.uint32 and w.shape == (nf * L // 32,)
    assert w[0] == 0b111 and w[1] == (0b11 << 30) and w[2] == 0b11 and w[3] == (0b111 << 29)
    assert np.array_equal(R.words_to_mask(w, L), m)
    # the float32 restatement through the same widening: one hot cell, dilate 1, wraps at bin 0
    P = np.ones((nf, L), dtype=np.float32)
    P[2, 0] = 100.0
    P[nf - 1, 5] = 29.0                                          # the last frame: 15.85 * 11/6 = 29.06
    f, mask, c = R.detect_from_power(P)
    assert f == 1 and c == 3 and np.flatnonzero(mask[2]).tolist() == [0, 1, 63] and not mask[nf - 1].any()
    P[nf - 1, 5] = 29.1
    assert R.detect_from_power(P)[2] == 6
    P[:] = 1.0                                                   # strictly above: equal cells are kept
    assert R.detect_from_power(P, thresh_db=1e-30)[2] == 0


def test_float32_oracle_stays_inside_the_borderline_cap():
    """Every case of the GPU table: the float32 oracle's mask equals the float64 mask but at cells whose
    P64 lies within 4 x its own power deviation of the threshold, at most BORDERLINE_CAP a block."""
    for name, c in R.CASES.items():
        bound = 4.0 * R.oracle_worst(name)[0]
        for rec in R.reference(name):
            near = R.borderline(rec, bound)
            assert near.sum() <= R.BORDERLINE_CAP, (name, int(near.sum()))
            if rec['count'] < 0:
                continue
            _, m32, c32 = R.detect_from_power(rec['P32'], **c['params'])
            if c32 < 0:
                continue
            diff = m32 != rec['mask']
            assert not (diff & ~R.widen(near, c['params']['dilate'])).any(), name


def _cfg(n=65536, frame=64, thresh=12.0, dilate=1, max_frac=0.5, keep=0):
    from gpsmi import _lib
    return _lib.TfxCfg(n, frame, thresh, dilate, max_frac, keep, 0, 0)


def test_abi_argument_errors_do_not_need_a_gpu():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(23) == C.sizeof(_lib.TfxCfg) == 32
    h = C.c_void_p(0xDEAD)
    assert lib.gpsmi_tfx_create(None, C.byref(h)) == -1                     # GPSMI_E_ARG
    assert lib.gpsmi_tfx_create(C.byref(_cfg()), None) == -1
    bad = [_cfg(thresh=float('nan')), _cfg(dilate=-2), _cfg(dilate=9), _cfg(max_frac=1.5), _cfg(max_frac=-0.1),
           _cfg(max_frac=float('nan')), _cfg(keep=2)]
    for cfg in bad:
        h = C.c_void_p(0xDEAD)
        assert lib.gpsmi_tfx_create(C.byref(cfg), C.byref(h)) == -1 and h.value is None
    for cfg, word in [(_cfg(frame=48), b'frame'), (_cfg(frame=512), b'frame'), (_cfg(n=1000), b'block_samples'),
                      (_cfg(n=896), b'block_samples'), (_cfg(n=65536 + 64), b'block_samples')]:
        h = C.c_void_p(0xDEAD)
        assert lib.gpsmi_tfx_create(C.byref(cfg), C.byref(h)) == -5 and h.value is None   # GPSMI_E_UNSUPPORTED
        assert word in lib.gpsmi_last_error()
    buf = np.zeros(16, dtype=np.complex64)
    assert lib.gpsmi_tfx_apply(None, _lib.ptr(buf), _lib.ptr(buf), 1, None, None, None) == -1
    assert lib.gpsmi_tfx_apply_dev(None, 16, 32, 1, None, None, None) == -1
    assert lib.gpsmi_tfx_set_input_format(None, 0) == -1
    assert lib.gpsmi_tfx_reset(None) == -1
    assert lib.gpsmi_tfx_last_ms(None, None) == -1
    assert lib.gpsmi_tfx_last_power(None, _lib.ptr(buf)) == -1
    assert lib.gpsmi_tfx_destroy(None) == 0


def test_python_wrapper_rejects_bad_arguments_without_a_gpu():
    from gpsmi.engine import Config, EngineError
    from gpsmi.tfexcision import SweepExcision, default_frame
    assert default_frame(2048) == 64 and default_frame(16368) == 32
    with pytest.raises(EngineError, match=r'\(-5\).*frame'):
        SweepExcision(Config(), frame=48)
    with pytest.raises(EngineError, match=r'\(-1\)'):
        SweepExcision(Config(), max_frac=1.5)
    with pytest.raises(EngineError, match=r'\(-1\)'):
        SweepExcision(Config(), thresh_db=float('nan'))


def test_conditioner_puts_the_stage_between_excision_and_blanking():
    """The order of the chain and which stage takes the raw format, with stand-ins for the handles."""
    from gpsmi import conditioning
    from gpsmi.engine import Config

    class Stub:
        def __init__(self, cfg, raw_u8=False, **kw):
            self.raw_u8, self.n, self.kw = raw_u8, cfg.ngps, kw

        def close(self):
            pass

    made = {}

    def stage(self, cls, arg, raw_u8, **kw):
        made[cls.__name__] = s = Stub(self.cfg, raw_u8, **kw)
        return s

    orig_stage = conditioning.Conditioner._stage
    orig_pin, orig_dev = conditioning.PinnedArray, conditioning.DeviceBuffer
    conditioning.Conditioner._stage = stage
    conditioning.PinnedArray = lambda *a, **k: None
    conditioning.DeviceBuffer = lambda *a, **k: None
    try:
        c = conditioning.Conditioner(Config(), True, excise=True, blank=True, sweep=True)
        assert [type(s) for s in c.stages] == [Stub] * 3
        assert c.stages == [made['Excision'], made['SweepExcision'], made['PulseBlanker']]
        assert [s.raw_u8 for s in c.stages] == [True, False, False] and c.sweeper is made['SweepExcision']
        c._pinned = None
        c = conditioning.Conditioner(Config(), True, blank=True, sweep=128)
        assert c.stages == [made['SweepExcision'], made['PulseBlanker']]
        assert [s.raw_u8 for s in c.stages] == [True, False] and made['SweepExcision'].kw == {'frame': 128}
        c._pinned = None
        c = conditioning.Conditioner(Config(), False, blank=True)
        assert c.sweeper is None and c.stages == [made['PulseBlanker']]
        c._pinned = None
    finally:
        conditioning.Conditioner._stage = orig_stage
        conditioning.PinnedArray, conditioning.DeviceBuffer = orig_pin, orig_dev
