"""The scope of the handles' events (csrc/gpsmi_event_scope.h): every event that
only orders one queue behind another, or carries a stamp, completes without writing back and
invalidating the caches.  What could go wrong is a consumer on another queue, or the host, reading a
stale line.  So the step of bench.py runs here 24 times -- replay_run_async, search_async behind
after(trk), replay_fetch_async, wait_prev -- with a different state table and different blocks in
every step (the expected bytes change from step to step), every output slot overwritten with a
pattern before it is refilled, and every record array and every peak table compared bytewise with
the closed loop / the search run alone.  The same through process_stream.

Shapes: 16 blocks x 12 channels, and 9 blocks x 5 channels (a partly filled channel group), each
with the span correlator's single-block form (what these sizes take by default: an event record
signals the correlator) and its batch form (span_single_max = 1: the dispatch's own stop event does,
as at the benchmark's 1024 blocks)."""
import numpy as np
import pytest

from conftest import scene_blocks

pytestmark = pytest.mark.gpu

STEPS = 24
FIRST = 5                       # the fixture scene's first tracked block
N_BLOCKS = 16 + STEPS - 1       # step k replays blocks [k, k + nb)


@pytest.fixture(scope='module')
def loops(golden_default):
    """The closed loop over N_BLOCKS blocks, with 12 and with 5 channels: per block the states at its
    start and its records.  Computed once, read by every test, never changed."""
    from gpsmi.engine import TrkEngine, STATE_DTYPE
    blocks = scene_blocks('default', FIRST, N_BLOCKS)
    out = {}
    for nch in (12, 5):
        eng = TrkEngine(max_ch=nch)
        for c, (sv, f0, d0) in enumerate(golden_default['trk_init'][:nch]):
            eng.open(c, int(sv), float(f0), int(d0))
        states = np.zeros((N_BLOCKS, nch), dtype=STATE_DTYPE)
        outs = []
        for i in range(N_BLOCKS):
            for c in range(nch):
                states[i, c] = eng.get_state(c)
            outs.append(eng.process(blocks[i]))
        eng.close()
        outs = np.array(outs)
        states.setflags(write=False)
        outs.setflags(write=False)
        out[nch] = (states, outs)
    return blocks, out


@pytest.fixture(scope='module')
def device_blocks(loops):
    from gpsmi.engine import DeviceBuffer
    blocks = loops[0]
    buf = DeviceBuffer(len(blocks) * blocks[0].nbytes)
    for i, b in enumerate(blocks):
        buf.upload(b, i * b.nbytes)
    yield buf
    buf.free()


@pytest.mark.parametrize('batch_form', [False, True], ids=['single', 'batch'])
@pytest.mark.parametrize('nb,nch', [(16, 12), (9, 5)])
def test_bench_step_reads_no_stale_line(loops, device_blocks, nb, nch, batch_form):
    from gpsmi.engine import AcqEngine, TrkEngine, PinnedArray, OUT_DTYPE, PEAK_DTYPE
    blocks, by_nch = loops
    states, outs = by_nch[nch]
    blk_bytes = blocks[0].nbytes
    eng = TrkEngine(max_ch=nch)
    if batch_form:
        eng.set_option('span_single_max', 1)
    acq = AcqEngine()
    prns = list(range(1, 33))
    freqs = [-5000.0 + 250.0 * i for i in range(41)]
    n = 2048
    # the search of step k reads block k: what it returns when nothing runs beside it
    want_acq = [acq.search((device_blocks.at(k * blk_bytes), n), prns, freqs, 1) for k in range(STEPS)]
    assert want_acq[0].tobytes() != want_acq[1].tobytes()
    pins = [PinnedArray((nb, nch), OUT_DTYPE) for _ in range(2)]
    apins = [PinnedArray((len(freqs), len(prns)), PEAK_DTYPE) for _ in range(2)]

    def expect(k):
        return outs[k:k + nb].tobytes()

    assert expect(0) != expect(1)
    try:
        for k in range(STEPS):
            if k > 0:
                acq.wait()
                assert apins[(k - 1) & 1].array.tobytes() == want_acq[k - 1].tobytes(), k
            pins[k & 1].array.view(np.uint8)[:] = 0xA0 + (k & 15)      # a different pattern each step
            apins[k & 1].array.view(np.uint8)[:] = 0xC0 + (k & 15)
            eng.replay_load(nb, states[k:k + nb], outs['delay_used'][k:k + nb])
            acq.after(eng)
            eng.set_timing(k % 3)
            eng.replay_run_async(device_blocks.at(k * blk_bytes), nb)
            acq.search_async(device_blocks.at(k * blk_bytes), n, prns, freqs, 1, apins[k & 1].array)
            eng.replay_fetch_async(pins[k & 1].array)
            eng.wait_prev()
            if k > 0:
                assert pins[(k - 1) & 1].array.tobytes() == expect(k - 1), k
        acq.wait()
        eng.wait()
        assert apins[(STEPS - 1) & 1].array.tobytes() == want_acq[STEPS - 1].tobytes()
        assert pins[(STEPS - 1) & 1].array.tobytes() == expect(STEPS - 1)
    finally:
        for p in pins + apins:
            p.free()
        acq.close()
        eng.close()


def test_bench_step_pipelined_under_one_table(loops, device_blocks):
    """replay_load waits for the runs in flight, so the steps above never overlap.  Here one table
    stays loaded, as in bench.py, and two steps are in flight at a time: the epilogue and the read-back
    of step k run beside the code-phase correlation of step k + 1.  The timing mode alternates."""
    from gpsmi.engine import AcqEngine, TrkEngine, PinnedArray, OUT_DTYPE, PEAK_DTYPE
    blocks, by_nch = loops
    nb, nch = 16, 12
    states, outs = by_nch[nch]
    eng = TrkEngine(max_ch=nch)
    eng.set_option('span_single_max', 1)
    acq = AcqEngine()
    prns = list(range(1, 33))
    freqs = [-5000.0 + 250.0 * i for i in range(41)]
    want_acq = acq.search((device_blocks.ptr, 2048), prns, freqs, 1).tobytes()
    want = outs[:nb].tobytes()
    pins = [PinnedArray((nb, nch), OUT_DTYPE) for _ in range(2)]
    apins = [PinnedArray((len(freqs), len(prns)), PEAK_DTYPE) for _ in range(2)]
    eng.replay_load(nb, states[:nb], outs['delay_used'][:nb])
    try:
        for k in range(STEPS):
            if k > 0:
                acq.wait()
                assert apins[(k - 1) & 1].array.tobytes() == want_acq, k
            pins[k & 1].array.view(np.uint8)[:] = 0xA0 + (k & 15)
            apins[k & 1].array.view(np.uint8)[:] = 0xC0 + (k & 15)
            acq.after(eng)
            eng.set_timing(k % 3)
            eng.replay_run_async(device_blocks.ptr, nb)
            acq.search_async(device_blocks.ptr, 2048, prns, freqs, 1, apins[k & 1].array)
            eng.replay_fetch_async(pins[k & 1].array)
            eng.wait_prev()
            if k > 0:
                assert pins[(k - 1) & 1].array.tobytes() == want, k
        acq.wait()
        eng.wait()
        assert apins[(STEPS - 1) & 1].array.tobytes() == want_acq
        assert pins[(STEPS - 1) & 1].array.tobytes() == want
    finally:
        for p in pins + apins:
            p.free()
        acq.close()
        eng.close()


@pytest.mark.parametrize('pinned_out', [True, False], ids=['pinned_out', 'pageable_out'])
def test_streamed_steps_read_no_stale_line(loops, golden_default, pinned_out):
    """32 blocks through process_stream from page-locked memory.  With a page-locked `out` the kernels
    store the records straight into it and the step's completion event is its last dispatch's own
    signal (in_done: host-visible, the host reads behind it with no copy in between)."""
    from gpsmi.engine import TrkEngine, PinnedArray, OUT_DTYPE
    blocks, by_nch = loops
    nch, nsteps, ring = 12, 32, 3
    _, outs = by_nch[nch]
    eng = TrkEngine(max_ch=nch)
    for c, (sv, f0, d0) in enumerate(golden_default['trk_init'][:nch]):
        eng.open(c, int(sv), float(f0), int(d0))
    iq = [PinnedArray(blocks[0].shape, np.complex64) for _ in range(ring)]
    pins = [PinnedArray((nch,), OUT_DTYPE) for _ in range(ring)]
    o = [p.array for p in pins] if pinned_out else [np.zeros(nch, dtype=OUT_DTYPE) for _ in range(ring)]
    try:
        for k in range(nsteps):
            # (the call before last has returned twice since: slot k % 3 was checked and is free)
            iq[k % ring].array[:] = blocks[k]
            o[k % ring].view(np.uint8)[:] = 0xA0 + (k & 15)
            eng.set_timing(k % 3)                   # (a streamed step takes no kernel-timing events, whatever is set)
            eng.process_stream(iq[k % ring].array, o[k % ring])
            if k >= 2:                              # the step of the call before last is complete
                assert o[(k - 2) % ring].tobytes() == outs[k - 2].tobytes(), k
        eng.wait()
        for k in (nsteps - 2, nsteps - 1):
            assert o[k % ring].tobytes() == outs[k].tobytes(), k
    finally:
        eng.close()
        for p in iq + pins:
            p.free()
