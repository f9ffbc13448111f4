"""The front-end stage without a GPU (gpsmi_fe_*, gpsmi/frontend.py): ABI, argument checks, the
refused configurations, the filter gpsmi_fe_design returns for the named configurations A-F, and
the numpy restatement (tests/fe_ref.py) on a known tone."""
import ctypes as C

import numpy as np
import pytest

import fe_ref as R


def _cfg(name, **kw):
    c = dict(R.CONFIGS[name])
    c.update(kw)
    return c


def _design(c):
    from gpsmi import frontend
    return frontend.design(c['fs_in'], c['fs_out'], c['fmt'], c['if_hz'], c.get('conjugate', False),
                           c['passband_hz'], c.get('atten_db', 60.0))


def test_struct_layout_and_exports():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(5) == C.sizeof(_lib.FeCfg) == 48
    covered = sum(C.sizeof(t) for _, t in _lib.FeCfg._fields_)
    assert covered == C.sizeof(_lib.FeCfg)                        # no implicit padding
    offs = [getattr(_lib.FeCfg, n).offset for n, _ in _lib.FeCfg._fields_]
    assert offs == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    for name in ('gpsmi_fe_design', 'gpsmi_fe_create', 'gpsmi_fe_destroy', 'gpsmi_fe_reset', 'gpsmi_fe_push',
                 'gpsmi_fe_push_dev', 'gpsmi_fe_flush', 'gpsmi_fe_last_ms'):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_argument_errors_before_any_gpu_call():
    from gpsmi import _lib, frontend
    lib = _lib.load()
    k, ph, h, n = C.c_int(), C.c_int(), C.c_void_p(0xBEEF), C.c_size_t()
    assert lib.gpsmi_fe_design(None, C.byref(k), C.byref(ph), None) == -1
    assert lib.gpsmi_fe_create(None, C.byref(h)) == -1
    good = frontend.fe_cfg(4_000_000, 2_048_000, 'sc16', max_out=1024)
    assert lib.gpsmi_fe_design(C.byref(good), None, C.byref(ph), None) == -1
    bad = [
        frontend.fe_cfg(0, 2_048_000, 'sc16'),
        frontend.fe_cfg(4_000_000, -1, 'sc16'),
        frontend.fe_cfg(4_000_000, 2_048_000, 'sc16', if_hz=float('nan')),
        frontend.fe_cfg(4_000_000, 2_048_000, 'sc16', passband_hz=-1.0),
        frontend.fe_cfg(4_000_000, 2_048_000, 'sc16', atten_db=5.0),
        frontend.fe_cfg(16_368_000, 2_048_000, 'r8', if_hz=4.092e6, conjugate=True),
    ]
    bad_fmt = frontend.fe_cfg(4_000_000, 2_048_000, 'sc16')
    bad_fmt.format = 9
    bad_flags = frontend.fe_cfg(4_000_000, 2_048_000, 'sc16')
    bad_flags.flags = 6
    for c in bad + [bad_fmt, bad_flags]:
        assert lib.gpsmi_fe_design(C.byref(c), C.byref(k), C.byref(ph), None) == -1
        h = C.c_void_p(0xBEEF)
        assert lib.gpsmi_fe_create(C.byref(c), C.byref(h)) == -1 and h.value is None
    no_out = frontend.fe_cfg(4_000_000, 2_048_000, 'sc16', max_out=0)
    h = C.c_void_p(0xBEEF)
    assert lib.gpsmi_fe_create(C.byref(no_out), C.byref(h)) == -1 and h.value is None
    assert lib.gpsmi_fe_push(None, None, 0, None, 0, C.byref(n)) == -1
    assert lib.gpsmi_fe_push_dev(None, None, 0, None, 0, C.byref(n)) == -1
    assert lib.gpsmi_fe_flush(None, None, 0, C.byref(n)) == -1
    assert lib.gpsmi_fe_reset(None) == -1
    assert lib.gpsmi_fe_last_ms(None, None) == -1
    assert lib.gpsmi_fe_destroy(None) == 0
    with pytest.raises(ValueError):
        frontend.fe_cfg(4_000_000, 2_048_000, 'u4')


@pytest.mark.parametrize('kw, what', [
    (dict(fmt='r8', fs_in=16_368_000, if_hz=4_092_000.0, fs_out=16_368_000, passband_hz=None), 'image'),
    (dict(fmt='r8', fs_in=16_368_000, if_hz=500_000.0, fs_out=2_048_000, passband_hz=None), 'image'),
    (dict(fmt='sc16', fs_in=1_000_000, if_hz=0.0, fs_out=2_048_000, passband_hz=None), '0.5 .. 64'),
    (dict(fmt='sc16', fs_in=200_000_000, if_hz=0.0, fs_out=2_048_000, passband_hz=None), '0.5 .. 64'),
    (dict(fmt='sc16', fs_in=4_000_000, if_hz=0.0, fs_out=2_048_000, passband_hz=1_100_000.0), 'passband'),
])
def test_unsupported_configurations(kw, what):
    from gpsmi import _lib, frontend
    lib = _lib.load()
    c = frontend.fe_cfg(kw['fs_in'], kw['fs_out'], kw['fmt'], kw['if_hz'], False, kw['passband_hz'], 60.0, 1024)
    k, ph = C.c_int(), C.c_int()
    assert lib.gpsmi_fe_design(C.byref(c), C.byref(k), C.byref(ph), None) == -5        # GPSMI_E_UNSUPPORTED
    assert what in lib.gpsmi_last_error().decode()
    h = C.c_void_p(0xBEEF)
    assert lib.gpsmi_fe_create(C.byref(c), C.byref(h)) == -5 and h.value is None


@pytest.mark.parametrize('name', sorted(R.CONFIGS))
def test_filter_meets_the_specification(name):
    """From the table alone: ripple <= 0.1 dB over |f| <= p; everything from the stop edge on (the
    nearest frequency that aliases, or images, into |f| <= p) down by >= 60 dB, the images of the
    phase interpolation at multiples of L fs_in included."""
    c = _cfg(name)
    K, L, T = _design(c)
    assert T.shape == (L + 1, K) and K % 2 == 0
    # linear phase: the prototype is symmetric about tau = 0 (row 0 tap m <-> tap K - 2 - m)
    np.testing.assert_allclose(T[0, :K - 1], T[0, K - 2::-1], rtol=0, atol=1e-7)
    fi, p, s = c['fs_in'], R.passband(c), R.stop_edge(c)
    assert s > p
    fp = np.linspace(-p, p, 801)
    Hp = R.response(T, K, L, fi, fp)
    db = 20 * np.log10(np.abs(Hp))
    assert db.max() - db.min() <= 0.1 and np.abs(db).max() <= 0.1, (db.min(), db.max())
    assert np.abs(Hp.imag).max() < 1e-6                    # zero phase: no group delay
    f1 = np.arange(s, 2 * max(fi, c['fs_out']), fi / K / 6)
    far = np.concatenate([m * L * fi + np.linspace(-2 * fi, 2 * fi, 801) for m in (1, 2, 3)])
    f = np.concatenate([f1, -f1, far, -far])
    f = f[np.abs(f) >= s]
    worst = 20 * np.log10(np.abs(R.response(T, K, L, fi, f)).max())
    assert worst <= -60.0, worst


def test_restatement_reproduces_a_tone():
    """Config B: a real cosine of amplitude A at IF + f -> a complex tone of amplitude A at f whose
    phase at output n is the input phase at t_n (zero group delay)."""
    c = _cfg('B')
    K, L, T = _design(c)
    fi, fo, A, f, phi = c['fs_in'], c['fs_out'], 0.3, 123_456.7, 0.4
    n_in = 60_000
    i = np.arange(n_in)
    x = A * np.cos(2 * np.pi * (c['if_hz'] + f) * i / fi + phi)
    raw = np.rint(x * 128.0).astype(np.int8)                  # quantised as the recording would be
    y = R.run(raw, c, K, L, T)
    P, Q = R.ratio(fi, fo)
    n = np.arange(len(y))
    want = (raw.astype(np.float64) / 128.0)
    # compare against the quantised input's own tone: least-squares amplitude and phase
    core = slice(K, len(y) - K)
    ref = np.exp(1j * (2 * np.pi * f * n / fo + phi))
    g = np.vdot(ref[core], y[core]) / np.vdot(ref[core], ref[core])
    assert abs(20 * np.log10(abs(g) / A)) <= 0.1, abs(g)
    assert abs(np.angle(g)) <= 2e-3, np.angle(g)
    assert np.abs(y[core] - A * ref[core]).max() <= 0.02 * A
    assert want.size == n_in and R.complete(K, P, Q, n_in) == len(y)
