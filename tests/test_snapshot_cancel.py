"""snapshot.measure(cancel=...) without a GPU: the scene check of the cancellation feature.  The
engine calls inside measure are answered by the float64 restatements (the deep search as deep_ref
states it, refine_ref, cancel_ref) on the collision scene of cancel_ref.py -- three satellites at
53 dB-Hz and PRN 3 at amplitude 0.00772 (30 dB-Hz) 2 Hz from PRN 4 modulo 1 kHz, 0.512 s -- so that
what test_gpu_snapshot_cancel.py asserts of the GPU path is known to hold for the algorithm itself:
without `cancel` PRN 3 is not among the records, with it PRNs 3, 4, 5 and 9 are and the absent PRNs
10 and 31 are not."""
import numpy as np
import pytest

import cancel_ref as R
from deep_ref import deep_shifts
from refine_ref import refine_ref


class RefEngine:
    """AcqEngine's search_deep on 'device' pairs (a numpy array stands for the pointer)."""
    raw_u8 = False

    def __init__(self, cs):
        self.cs = cs

    def last_ms(self):
        return 0.0

    def set_input_format(self, raw):
        assert not raw

    def search_deep(self, iq, prns, freqs, n_coh, n_seg, f_offset=0.0):
        from gpsmi._lib import PEAK_DTYPE
        cs = self.cs
        x = iq[0].arr[:iq[1]].astype(np.complex128)
        assert len(x) == n_seg * n_coh * cs
        t = (np.arange(n_coh * cs) + 1.0) / (1000.0 * cs)
        reps = [np.conj(np.fft.fft(R.replica64(p, cs))) for p in prns]
        m = deep_shifts(freqs, n_coh, n_seg, cs, f_offset=f_offset)
        out = np.zeros((len(freqs), len(prns)), PEAK_DTYPE)
        for b, f in enumerate(freqs):
            w = x.reshape(n_seg, n_coh * cs) * np.exp(-2j * np.pi * f * t)[None, :]
            spec = np.fft.fft(w.reshape(n_seg, n_coh, cs).sum(axis=1), axis=1)
            for j, rep in enumerate(reps):
                mag = np.abs(np.fft.ifft(spec * rep[None, :], axis=1))
                surf = np.mean([np.roll(mag[s], -int(m[b, s])) for s in range(n_seg)], axis=0)
                out[b, j] = (int(np.argmax(surf)), surf.max(), surf.mean(), surf.std())
        return out


class Buffer:
    """Stands for engine.DeviceBuffer: `ptr` is the object itself."""

    def __init__(self, nbytes, device=0):
        self.arr = np.zeros(nbytes // 8, np.complex64)
        self.ptr = self

    def free(self):
        pass


class RefAcquisition:
    def __init__(self):
        from gpsmi.engine import Config
        self.cfg = Config()
        self.engine = RefEngine(self.cfg.code_samples)

    def refineHits(self, data, found, f_offset=0.0):
        from gpsmi._lib import REFINE_OUT_DTYPE
        cs = self.cfg.code_samples
        x = data[0].arr[:data[1]]
        n_ms = ((len(x) - 1) // cs - 2) // 20 * 20
        ref, _, _ = refine_ref(x, [(s, f, d) for _, s, f, d in found], n_ms, cs, f_offset=f_offset)
        out = np.zeros(len(ref), REFINE_OUT_DTYPE)
        for name in REFINE_OUT_DTYPE.names:
            out[name] = ref[name]
        return out

    def cancelHits(self, data, rec, f_offset=0.0, out=None):
        order = np.argsort(-rec['cn0_dbhz'], kind='stable')
        sats = [(int(rec['prn'][i]), float(rec['f_hz'][i]), float(rec['code_phase'][i])) for i in order]
        y, res, _, _ = R.cancel_ref(data[0].arr[:data[1]], sats, self.cfg.code_samples, f_offset=f_offset)
        out.arr[:] = y.astype(np.complex64)
        return out, res


@pytest.fixture(scope='module')
def scene():
    from gpsmi.synth import raw_to_c64
    buf = Buffer(0)
    buf.arr = raw_to_c64(R.collision_raw())
    return buf


def test_scene_check(scene, monkeypatch):
    from gpsmi import engine, snapshot as S
    monkeypatch.setattr(engine, 'DeviceBuffer', Buffer)
    acq = RefAcquisition()
    dev = (scene, len(scene.arr))
    st0, st1 = {}, {}
    before = S.measure(acq, dev, prns=R.COLLISION_PRNS, source='refine', stats=st0)
    after = S.measure(acq, dev, prns=R.COLLISION_PRNS, source='refine', stats=st1, cancel=True)
    for name, meas, st in (('without', before, st0), ('with cancel', after, st1)):
        print(name, [(int(m['prn']), round(float(m['code_phase']), 2), round(float(m['f_hz']), 1),
                      round(float(m['cn0_dbhz']), 1)) for m in meas])
        print('  found', [(round(h[0], 1), h[1], h[2], h[3]) for h in st['found']])
        print('  refined', [(int(r['prn']), int(r['confirmed']), round(float(r['f_hz']), 1),
                             round(float(r['code_phase']), 2), round(float(r['cn0_dbhz']), 1)) for r in st['refined']])
    assert 'cancelled' not in st0
    assert 3 not in before['prn'] and {4, 5, 9} <= set(before['prn'].tolist())
    assert after['prn'].tolist() == [3, 4, 5, 9]
    weak = after[0]
    p, f, d = R.COLLISION_WEAK
    assert abs(weak['code_phase'] - R.true_tau(f, d)) <= 0.25 and abs(weak['f_hz'] - f) <= 5.0
    assert sorted(st1['cancelled']['prn'].tolist()) == [4, 5, 9]
    ratio = st1['cancelled']['energy_removed'] / st1['cancelled']['energy_in']
    print('removed / in', ratio)
    assert np.all((ratio > 0.02) & (ratio < 0.2))
    # the kept records are the first pass's, untouched
    for prn in (4, 5, 9):
        assert before[before['prn'] == prn].tobytes() == after[after['prn'] == prn].tobytes()
