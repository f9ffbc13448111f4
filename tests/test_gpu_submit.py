"""gpsmi_trk_process_stream through the handle's submission thread (option "stream_thread" = 1, at
"stream_depth" 2 and 3) against the same steps made by the caller's own thread ("stream_thread" = 0):
the same launches in the same order, so every record and the final state rows are bytewise equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NB, NCH = 24, 2


def test_submission_thread_equals_callers_thread():
    from gpsmi import synth
    from gpsmi.engine import Config, TrkEngine, PinnedArray, OUT_DTYPE
    cfg = Config(code_samples=2048, n_cyc=8)
    sc = synth.default_scene(NCH, seed=5, code_samples=2048, n_cyc=8)
    iq = PinnedArray((NB, cfg.ngps), np.complex64)       # every block in memory of its own: none is rewritten
    for b in range(NB):
        iq.array[b] = sc.block(b)
    results = []
    for thread, depth in ((0, 2), (1, 2), (1, 3)):
        eng = TrkEngine(cfg, max_ch=NCH, prns=[s.prn for s in sc.sats])
        eng.set_option('stream_thread', thread)
        eng.set_option('stream_depth', depth)
        for c, s in enumerate(sc.sats):
            eng.open(c, s.prn, round(s.doppler / 200.0) * 200.0, int(round(s.delay)) % 2048)
        out = PinnedArray((NB, NCH), OUT_DTYPE)
        out.array.view(np.uint8)[:] = 0xAB
        for b in range(NB):
            eng.process_stream(iq.array[b], out.array[b])
        eng.wait()
        assert eng.get_option('stat_stream_steps') == NB, (thread, depth)
        state = b''.join(eng.get_state(c).tobytes() for c in range(NCH))
        results.append((out.array.tobytes(), state))
        eng.close()
        out.free()
    iq.free()
    assert results[0][0] != b'\xab' * len(results[0][0])           # (the records were written)
    for k, (thread, depth) in ((1, (1, 2)), (2, (1, 3))):
        assert results[k][0] == results[0][0], f'records differ: stream_thread {thread}, stream_depth {depth}'
        assert results[k][1] == results[0][1], f'state rows differ: stream_thread {thread}, stream_depth {depth}'
