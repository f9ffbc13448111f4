"""Null steering without a GPU: the float64 restatement of the contract (tests/nul_ref.py, what
gpsmi_nul_* is held to) on the synthetic array scenes, and the argument errors of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import nul_ref as R

from nul_ref import A4, JAM_SINE, JN_DB, array_scene


def test_array_scene_levels_and_streams():
    from gpsmi import synth_array as SA
    arr, clean = array_scene(), array_scene(False)
    sc = arr.scene
    # antenna 0 of the clean scene at unit steering is the single-antenna scene itself
    assert clean.scale == 1.0 and np.array_equal(clean.block_raw(1)[0], sc.block_raw(1))
    # the jammed scene is scaled down until the 8 bits clip fewer than 1e-3 of the samples
    assert arr.scale < 0.1
    assert arr.clip_fraction(0) < 1e-3 and arr.clip_fraction(1) < 1e-3
    sat, noise, jam = arr.parts(0)
    assert sat.shape == noise.shape == jam.shape == (A4, sc.ngps)
    p_n = np.mean(np.abs(noise) ** 2, axis=1)
    assert np.allclose(p_n, (arr.scale * sc.noise_sigma) ** 2, rtol=0.02)
    assert np.allclose(10 * np.log10(np.mean(np.abs(jam) ** 2, axis=1) / p_n), JN_DB, atol=0.2)
    # the noise is independent per antenna, the jammer is one waveform with a phase per antenna
    c = np.corrcoef(noise)
    assert np.abs(c - np.eye(A4)).max() < 0.02
    assert np.allclose(jam[2], jam[0] * SA.ula_steering(A4, [JAM_SINE])[2, 0])
    # a tone field comes from the same counter-based generator: any block on its own, the same bits
    tones = SA.ArrayScene(sc, arr.steering, [SA.Jammer(steering=np.ones(A4), kind='tones',
                                                       tones=[-300e3, 11e3, 412.5e3])])
    z = tones.jammer_parts(3, 4096)
    assert np.array_equal(z, tones.jammer_parts(3, 4096))
    assert np.allclose(np.mean(np.abs(z) ** 2), tones.jammer_power(tones.jammers[0]), rtol=0.05)


def test_reference_nulls_the_jammer_and_keeps_the_satellites():
    """Jammer suppression and every satellite's SNR against the unjammed antenna 0, measured from the
    rendered components run through the block's own weights.  Measured on blocks 0 and 1: suppression
    66.1 and 71.6 dB; satellite SNR -1.4, +1.3, -1.4, +1.8, -0.2, -10.3, +1.9, -0.2 dB (the sixth
    stands 3 degrees from the jammer and goes with it)."""
    arr = array_scene()
    sc = arr.scene
    ref = R.NullRef(sc.ngps, A4)
    for b in (0, 1):
        y, flag, gain_db, w = ref.process(arr.block(b))
        assert flag == 1 and 27.0 < gain_db < 28.5            # (30 dB up, less what the 8 bits add)
        assert w[0] == 1.0
        _, noise, jam = arr.parts(b)
        wc = np.conj(w)[:, None]
        left = (wc * jam).sum(axis=0)
        supp = 10 * np.log10(np.mean(np.abs(jam[0]) ** 2) / np.mean(np.abs(left) ** 2))
        assert supp >= 66.05 - 1.0, supp
        rest = np.mean(np.abs((wc * (noise + jam)).sum(axis=0)) ** 2)
        sp = arr.scale * arr.sat_parts(b)
        d = []
        for s in range(len(sc.sats)):
            out = np.mean(np.abs((wc * (arr.steering[:, s][:, None] * sp[s][None, :])).sum(axis=0)) ** 2)
            d.append(10 * np.log10((out / rest) / (np.mean(np.abs(sp[s]) ** 2) / np.mean(np.abs(noise[0]) ** 2))))
        print(f'block {b}: suppression {supp:.1f} dB, satellite SNR against unjammed antenna 0:', np.round(d, 2))
        assert sorted(d)[1] > -2.5 and min(d) > -12.0         # (one satellite near the null)
        assert 10 * np.log10(np.mean(np.abs(y) ** 2) / np.mean(np.abs(arr.block(b)[0]) ** 2)) < -26.0


def test_clean_scene_passes_antenna_0_through():
    clean = array_scene(False)
    ref = R.NullRef(clean.ngps, A4)
    xs = np.concatenate([clean.block(b) for b in range(3)], axis=1)
    y, flags, gain, w = ref.run(xs)
    assert not flags.any() and (gain < 1.0).all()
    assert y.tobytes() == xs[0].tobytes()
    assert np.array_equal(w, np.tile(np.eye(A4)[0], (3, 1)))
    # raw input: the decode of antenna 0
    raw = np.concatenate([clean.block_raw(b) for b in range(3)], axis=1)
    y2, flags2, _, _ = ref.run(raw)
    assert not flags2.any() and y2.tobytes() == R.decode(raw[0]).tobytes() == y.tobytes()


def _gain(jn_db, n=2048, A=2, seed=5):
    rng = np.random.default_rng(seed)
    x = R.noisy_block(rng, A, n, 1, jn_db).astype(np.complex64)
    return x, float(R.NullRef(n, A, min_gain_db=0.01).process(x)[2])


def block_with_gain(target_db, n=2048, A=2, seed=5):
    """A block whose predicted gain is target_db within 0.05 dB: the jammer's level by bisection."""
    lo, hi = -20.0, 40.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        x, g = _gain(mid, n, A, seed)
        if abs(g - target_db) < 0.05:
            return x
        lo, hi = (mid, hi) if g < target_db else (lo, mid)
    raise AssertionError('no such level')


def test_threshold_takes_the_side_it_should():
    n = 2048
    for min_db in (0.0, 6.0):                                  # (0: the default, 3 dB)
        t = 3.0 if min_db == 0.0 else min_db
        ref = R.NullRef(n, 2, min_gain_db=min_db)
        below, above = block_with_gain(t - 1.0), block_with_gain(t + 1.0)
        y, flag, g, w = ref.process(below)
        assert flag == 0 and abs(g - (t - 1.0)) < 0.06 and y.tobytes() == below[0].tobytes()
        assert np.array_equal(w, [1.0, 0.0])
        y, flag, g, w = ref.process(above)
        assert flag == 1 and abs(g - (t + 1.0)) < 0.06 and w[0] == 1.0 and abs(w[1]) > 0.1
        assert y.tobytes() == R.combine(above, w).tobytes() != above[0].tobytes()


def test_degenerate_blocks():
    n, A = 4096 + 32, 3
    ref = R.NullRef(n, A)
    y, flag, g, w = ref.process(np.zeros((A, n), dtype=np.complex64))
    assert flag == 0 and g == 0 and not y.any() and np.array_equal(w, [1, 0, 0])
    # exact copies: singular without the loading, a deep null with it (w sums the others against 0)
    rng = np.random.default_rng(2)
    x = np.tile(R.cgauss(rng, n).astype(np.complex64), (A, 1))
    y, flag, g, w = ref.process(x)
    assert flag == 1 and g > 50.0
    assert abs(1.0 + np.conj(w[1:]).sum()) < 1e-5 and np.abs(y).max() < 1e-4 * np.abs(x).max()
    # the covariance in the stated order equals the plain one to float64 rounding
    x = R.noisy_block(rng, A, n, 2).astype(np.complex64)
    X = x.astype(np.complex128)
    C, Cp = R.covariance(x), X @ X.conj().T
    assert np.abs(C - Cp).max() <= 1e-13 * np.abs(Cp).max()
    assert np.array_equal(C, C.conj().T) and not C.imag.diagonal().any()


def test_restatement_against_plain_numpy():
    rng = np.random.default_rng(3)
    for A, n, J in ((2, 2048, 1), (5, 4128, 4), (8, 6144, 3)):
        x = R.noisy_block(rng, A, n, J).astype(np.complex64)
        y, flag, g, w = R.NullRef(n, A).process(x)
        yp, fp, gp, wp = R.plain(x, n)
        assert flag == fp == 1 and abs(float(g) - float(gp)) < 1e-4
        assert np.abs(w - wp).max() < 1e-9
        assert np.abs(y - yp).max() < 1e-5 * np.abs(x).max()


def _nul_cfg(n=65536, A=4, load=0.0, min_gain_db=0.0):
    from gpsmi import _lib
    return _lib.NulCfg(n, A, load, min_gain_db, 0, 0)


def test_abi_argument_errors_do_not_need_a_gpu():
    """(nb <= 0 on a live handle and overlapping buffers: tests/test_gpu_nulling.py, the checks need
    a handle's block length.)"""
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(21) == C.sizeof(_lib.NulCfg) == 24
    assert lib.gpsmi_abi_sizeof(20) == -1 and lib.gpsmi_abi_sizeof(22) == -1
    h = C.c_void_p(0xDEAD)
    assert lib.gpsmi_nul_create(None, C.byref(h)) == -1                     # GPSMI_E_ARG
    assert lib.gpsmi_nul_create(C.byref(_nul_cfg()), None) == -1
    nan = float('nan')
    bad = [_nul_cfg(A=a) for a in (1, 9, 0, -4)]
    bad += [_nul_cfg(n=n) for n in (2047, 2080 - 32 + 1, 0, -32, 1024, 2048 + 16, (1 << 24) + 32)]
    bad += [_nul_cfg(load=nan), _nul_cfg(load=-1e-3), _nul_cfg(min_gain_db=nan), _nul_cfg(min_gain_db=-3.0)]
    for cfg in bad:
        h = C.c_void_p(0xDEAD)
        assert lib.gpsmi_nul_create(C.byref(cfg), C.byref(h)) == -1 and h.value is None
    assert b'antennas' in lib.gpsmi_last_error() or b'min_gain_db' in lib.gpsmi_last_error()
    buf = np.zeros(16, dtype=np.complex64)
    for nb in (1, 0, -1):
        assert lib.gpsmi_nul_apply(None, _lib.ptr(buf), _lib.ptr(buf), nb, None, None, None) == -1
        assert lib.gpsmi_nul_apply_dev(None, 16, 32, nb, None, None, None) == -1
    assert lib.gpsmi_nul_set_input_format(None, 0) == -1
    assert lib.gpsmi_nul_last_ms(None, None) == -1
    assert lib.gpsmi_nul_destroy(None) == 0


def test_python_wrapper_rejects_bad_arguments_without_a_gpu():
    from gpsmi.conditioning import Conditioner
    from gpsmi.engine import Config, EngineError
    from gpsmi.nulling import NullSteer
    for kw in (dict(antennas=1), dict(antennas=9), dict(load=float('nan')), dict(min_gain_db=-1.0)):
        with pytest.raises(EngineError, match=r'\(-1\)'):
            NullSteer(Config(), **kw)
    with pytest.raises(ValueError, match='antennas'):
        Conditioner(Config(), False, null=True)
    with pytest.raises(ValueError, match='antennas'):
        Conditioner(Config(), False, antennas=4)
    c = Conditioner(Config(), True)                           # the defaults: today's empty chain
    assert not c and c.out_raw_u8 and c.nuller is None and c.antennas == 1


def test_array_files_are_read_in_step(tmp_path):
    from gpsmi import ingest
    from gpsmi.engine import Config
    clean = array_scene(False)
    paths = [str(tmp_path / f'ant{a}.bin') for a in range(A4)]
    blocks = [clean.block_raw(b, 4096) for b in range(3)]
    cfg = Config(code_samples=2048, n_cyc=2)
    for a, p in enumerate(paths):
        with open(p, 'wb') as f:
            for x in blocks[:3 if a != 2 else 2]:              # (channel 2 is one block short)
                x[a].astype('<u2').tofile(f)
    with ingest.open_blocks(paths[0], cfg, antennas=paths[1:]) as (source, raw_u8):
        got = list(source)
    assert raw_u8 and len(got) == 2
    assert all(g.shape == (A4, 4096) and np.array_equal(g, x) for g, x in zip(got, blocks))
    with ingest.open_blocks(paths[0], cfg) as (source, raw_u8):   # without the keyword: as before
        assert raw_u8 and np.array_equal(next(iter(source)), blocks[0][0])
    with pytest.raises(ValueError, match='own format'):
        with ingest.open_blocks(paths[0], cfg, frontend={'fmt': 'sc8'}, antennas=paths[1:]):
            pass
