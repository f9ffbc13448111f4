"""GPU: strong-satellite cancellation (gpsmi_acq_cancel / AcqEngine.cancel) against the float64
restatement (cancel_ref.py), its bit-for-bit properties, the equivalence of its inputs and entry
points, the noise-free depth of the CPU test on the GPU's output, and what it leaves of the handle.

Shapes: n = 5 * 2048 + 123 at 2048 and one block of 130944 at 16368; satellites of both Doppler
signs; code starts within a sample of 0 (a first window of one sample: skipped), 14.5 (15 samples:
skipped), 15.5 (exactly min_window = 16: processed), just below cs, and negative.

Tolerances against the restatement: the GPU sums in float32, takes its carrier from 24 bits of an
integer phase and writes float32, so the deviations were measured on the first GPU run (MI355X, the
largest over all cases of a code length) and are asserted at four times that, under the hard cap
of 1e-4 (70 dB below an amplitude-0.11 satellite); the measured values stand beside each constant
and in DESIGN.md 4.2j."""
import ctypes as C
import functools

import numpy as np
import pytest

import cancel_ref as R
from test_gpu_acq_noncoherent import CFG, _same, _upload

pytestmark = pytest.mark.gpu

CAP = 1e-4
# asserted = 4 x the largest deviation measured on the first GPU run        measured
TOL = {2048: dict(out=4 * 2.689e-07,         # max |y - y_ref| / rms(x)      2.689e-07 (three satellites)
                  coef=4 * 3.879e-07),       # max |c - c_ref| / max |c_ref| 3.879e-07 (tau 14.5)
       16368: dict(out=4 * 3.987e-07,        #                               3.987e-07 (tau 0.3)
                   coef=4 * 2.533e-07)}      #                               2.533e-07 (three satellites)
assert all(v <= CAP for t in TOL.values() for v in t.values())
ENERGY_RTOL = 1e-5

N = {2048: 5 * 2048 + 123, 16368: 130944}


def scene_sats(cs):
    """(prn, Doppler, delay): code starts 15.7 samples in, just below cs, and in mid-period."""
    return ((4, 3094.0, 15.7), (5, -4321.0, cs - 0.4), (9, 400.0, 1347.4 * cs / 2048.0))


def cases(cs):
    k = cs / 2048.0
    return {'three': [(4, 3096.0, 15.5), (5, -4319.0, cs - 0.3), (9, 402.0, 1347.4 * k - cs)],
            'skip1': [(4, 3094.0, 0.3)],
            'skip15': [(5, -4321.0, 14.5)],
            'negative': [(9, 400.0, -0.4)],
            'none': []}


@functools.lru_cache(maxsize=None)
def scene_raw(cs):
    from gpsmi import synth
    sats = [synth.Sat(prn=p, doppler=f, delay=d, amp=0.11, phase0=0.4 * i)
            for i, (p, f, d) in enumerate(scene_sats(cs))]
    sc = synth.Scene(sats=sats, seed=23, noise_sigma=0.35, code_samples=cs, n_cyc=CFG[cs]['n_cyc'])
    out = sc.block_raw(0, n=N[cs])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_c64(cs):
    from gpsmi.synth import raw_to_c64
    out = raw_to_c64(scene_raw(cs))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(cs, case):
    return R.cancel_ref(scene_c64(cs), cases(cs)[case], cs)


@pytest.fixture(scope='module')
def engines():
    from gpsmi.engine import AcqEngine, Config
    made = {}

    def get(cs, raw):
        if (cs, raw) not in made:
            e = AcqEngine(Config(**CFG[cs]))
            e.set_input_format(raw)
            made[cs, raw] = e
        return made[cs, raw]
    yield get
    for e in made.values():
        e.close()


def data_of(cs, raw):
    return scene_raw(cs) if raw else scene_c64(cs)


def on_device(e, data, sats, in_place=False, coef=False):
    """AcqEngine.cancel on device-resident data -> (y, records[, coef]) downloaded."""
    from gpsmi.engine import DeviceBuffer
    d_in = _upload(data)
    d_out = None if in_place else DeviceBuffer(8 * len(data))
    try:
        res = e.cancel((d_in.ptr, len(data)), sats, out=None if in_place else d_out.ptr, coef=coef)
        y = (d_in if in_place else d_out).download(np.complex64, len(data))
        return (y,) + tuple(res[1:])
    finally:
        d_in.free()
        if d_out is not None:
            d_out.free()


MEASURED = {2048: dict(out=0.0, coef=0.0), 16368: dict(out=0.0, coef=0.0)}

SHAPES = [(2048, raw, c) for raw in (False, True) for c in ('three', 'skip1', 'skip15', 'negative', 'none')] + \
         [(16368, False, 'three'), (16368, True, 'three'), (16368, False, 'skip1')]


@pytest.mark.parametrize('cs,raw,case', SHAPES, ids=lambda v: str(v))
def test_against_the_restatement(engines, cs, raw, case):
    e = engines(cs, raw)
    sats = cases(cs)[case]
    x0 = scene_c64(cs)
    y_ref, rec_ref, coef_ref, done = reference(cs, case)
    y, rec, coef = e.cancel(data_of(cs, raw), sats, coef=True)
    assert e.last_ms() > 0 or not len(sats)
    # the diagnostics
    assert rec['prn'].tolist() == [s[0] for s in sats]
    assert np.array_equal(rec['n_windows'], rec_ref['n_windows'])
    assert np.array_equal(rec['n_skipped'], rec_ref['n_skipped'])
    assert rec['n_skipped'].tolist() == {'three': [0, 0, 0], 'skip1': [1], 'skip15': [1], 'negative': [0],
                                         'none': []}[case]
    np.testing.assert_allclose(rec['energy_in'], rec_ref['energy_in'], rtol=ENERGY_RTOL)
    np.testing.assert_allclose(rec['energy_removed'], rec_ref['energy_removed'], rtol=ENERGY_RTOL)
    assert coef.shape == coef_ref.shape
    # bit for bit: what no processed window holds is the decoded / copied input
    untouched = ~done.any(axis=0) if len(sats) else np.ones(len(x0), bool)
    _same(y[untouched], x0[untouched])
    if case.startswith('skip'):
        assert untouched.sum() == {'skip1': 1, 'skip15': 15}[case] and untouched[0]
    if not len(sats):
        return
    # the numbers
    rms = np.sqrt(np.mean(np.abs(x0.astype(np.complex128)) ** 2))
    d_out = np.abs(y - y_ref).max() / rms
    d_coef = np.abs(coef - coef_ref).max() / np.abs(coef_ref).max()
    print('deviations cs %d raw %d %s: out %.3e  coef %.3e' % (cs, raw, case, d_out, d_coef))
    MEASURED[cs]['out'] = max(MEASURED[cs]['out'], d_out)
    MEASURED[cs]['coef'] = max(MEASURED[cs]['coef'], d_coef)
    print('largest so far cs %d: out %.3e  coef %.3e' % (cs, MEASURED[cs]['out'], MEASURED[cs]['coef']))
    assert np.all(coef[coef_ref == 0] == 0)              # skipped windows, and past a satellite's last
    assert d_out <= TOL[cs]['out'] and d_coef <= TOL[cs]['coef']
    # the same bytes again
    y2, rec2, coef2 = e.cancel(data_of(cs, raw), sats, coef=True)
    _same(y, y2), _same(rec, rec2), _same(coef, coef2)


@pytest.mark.parametrize('cs,raw', [(2048, False), (2048, True), (16368, False), (16368, True)])
def test_entry_points_and_formats_agree(engines, cs, raw):
    """Host and device memory, out of place and in place, raw and complex64 input: one result."""
    e = engines(cs, raw)
    sats = cases(cs)['three']
    y, rec, coef = e.cancel(data_of(cs, raw), sats, coef=True)
    yd, recd, coefd = on_device(e, data_of(cs, raw), sats, coef=True)
    _same(y, yd), _same(rec, recd), _same(coef, coefd)
    into = np.zeros(N[cs], np.complex64)
    assert e.cancel(data_of(cs, raw), sats, out=into)[0] is into
    _same(into, y)
    if raw:
        yc, recc = engines(cs, False).cancel(scene_c64(cs), sats)
        _same(y, yc), _same(rec, recc)
        with pytest.raises(ValueError):
            e.cancel((C.c_void_p(1 << 20), N[cs]), sats)          # raw input has no in-place form
    else:
        yi, reci = on_device(e, data_of(cs, raw), sats, in_place=True)
        _same(y, yi), _same(rec, reci)


@pytest.mark.parametrize('raw', [False, True])
def test_no_satellite_decodes_or_copies(engines, raw):
    from gpsmi.engine import DeviceBuffer, unpack_u8iq
    e = engines(2048, raw)
    y, rec = e.cancel(data_of(2048, raw), [])
    assert len(rec) == 0
    _same(y, scene_c64(2048))
    yd, _ = on_device(e, data_of(2048, raw), [])
    _same(yd, y)
    if raw:
        d_raw, d_out = _upload(scene_raw(2048)), DeviceBuffer(8 * N[2048])
        try:
            unpack_u8iq(d_out.ptr, d_raw.ptr, N[2048])
            _same(d_out.download(np.complex64, N[2048]), y)
        finally:
            d_raw.free(), d_out.free()


@pytest.mark.parametrize('doppler', R.DEPTH_DOPPLERS)
def test_noise_free_depth(engines, doppler):
    """The thresholds of test_cancel.py on the GPU's output."""
    e = engines(2048, False)
    x, tau, prn = R.depth_scene(doppler)
    for df, dt, bound in R.DEPTH_CASES:
        y, rec = e.cancel(x.astype(np.complex64), [(prn, doppler + df, tau + dt)])
        db = R.residual_db(y, x)
        print('doppler %+6.0f  %4.1f Hz %4.2f sample off: residual %6.1f dB (bound %.0f)' % (doppler, df, dt, db, bound))
        assert rec['n_skipped'][0] == 0 and db <= bound


@pytest.mark.parametrize('cs', [2048, 16368])
def test_idempotent(engines, cs):
    """One satellite's cancellation is a projection per window: applied again with the same
    parameters it finds nothing.  (Several satellites in a row are not one projection -- their bases
    are not orthogonal, taking out the second puts back a little of the first -- so each is applied
    twice on its own: the one with the 16-sample first window, the one near cs, the negative one.)"""
    e = engines(cs, False)
    rms = np.sqrt(np.mean(np.abs(scene_c64(cs).astype(np.complex128)) ** 2))
    for sat in cases(cs)['three']:
        y, rec = e.cancel(scene_c64(cs), [sat])
        y2, rec2 = e.cancel(y, [sat])
        d = np.abs(y2 - y).max() / rms
        print('second application cs %d prn %d: %.3e of rms, removes %.3e of the energy'
              % (cs, sat[0], d, rec2['energy_removed'][0] / rec2['energy_in'][0]))
        assert rec['n_skipped'][0] == 0 and d <= TOL[cs]['out']


def test_refusals_leave_the_handle_usable():
    """What needs the handle to be refused -- a PRN without a replica, buffers that overlap -- and
    that a search returns the same table before and after any of it."""
    from gpsmi import _lib
    from gpsmi.engine import AcqEngine, Config, DeviceBuffer, EngineError
    e = AcqEngine(Config(**CFG[2048]))
    x = scene_c64(2048)
    prns, freqs = [4, 5, 9, 11], [400.0, 3000.0, -4400.0]
    n_search = 5 * 2048
    try:
        before = e.search_deep(x[:n_search], prns, freqs, 1, 5)
        y, rec = e.cancel(x, cases(2048)['three'])
        _same(e.search_deep(x[:n_search], prns, freqs, 1, 5), before)
        # a PRN whose time-domain replica the handle never got: the library's own check
        sat = np.zeros(1, _lib.CANCEL_SAT_DTYPE)
        sat[0] = (17, 0, 100.0, 3.0)
        out, o = np.zeros(len(x), np.complex64), np.zeros(1, _lib.CANCEL_OUT_DTYPE)
        rc = e.lib.gpsmi_acq_cancel(e.h, _lib.ptr(x), len(x), _lib.ptr(sat), 1, None, _lib.ptr(out), _lib.ptr(o), None)
        assert rc == -3 and 'PRN 17' in e.lib.gpsmi_last_error().decode()
        for bad in ([(4, 0.0, 0.0), (4, 1.0, 1.0)], [(4, np.nan, 0.0)], [(4, 0.0, np.inf)], [(p, 0.0, 0.0) for p in range(1, 34)]):
            with pytest.raises(EngineError):
                e.cancel(x, bad)
        buf = DeviceBuffer(8 * len(x) + 64)
        try:
            buf.upload(x)
            with pytest.raises(EngineError, match='overlap'):
                e.cancel((buf.ptr, len(x)), cases(2048)['three'], out=buf.at(8))
            e.set_input_format(True)
            with pytest.raises(EngineError, match='overlap'):
                e.cancel((buf.ptr, len(x)), cases(2048)['three'], out=buf.ptr)
            e.set_input_format(False)
            _same(buf.download(np.complex64, len(x)), x)          # nothing was written
        finally:
            buf.free()
        y2, rec2 = e.cancel(x, cases(2048)['three'])
        _same(y2, y), _same(rec2, rec)
        _same(e.search_deep(x[:n_search], prns, freqs, 1, 5), before)
    finally:
        e.close()
