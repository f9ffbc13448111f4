"""GPU: a handle that is used again gives what a fresh handle gives.

Every handle keeps its device buffers between calls and lets them grow to what a call needs
(csrc/gpsmi_devmem.h).  A stale capacity -- a buffer believed larger than it is, or shared between
two entry points that size it differently -- shows as a result that depends on what the handle did
before.  So one handle of each kind is driven through a sequence that grows, shrinks and regrows
every scratch buffer and crosses the entry points that share buffers, and each call's outputs are
compared byte for byte with the same call on a fresh handle (fresh handles are what the
reference-pinned tests of each entry point cover).  The shapes are the smallest the entry points
accept; the inputs are a fixed pseudo-random scene, since only equality is asked."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P1, P2, P3 = 3, 11, 22
SATS = [(P1, 0.0, 300.0), (P2, 0.0, 1200.0)]       # _scene's satellites as cancel takes them: (prn, f_hz, tau)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))      # (bytes: NaN fields compare too)


def _same_all(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        _same(x, y)


def _scene(cs, n_ms, seed):
    """P1 and P2 at zero Doppler over noise, as complex64 and as the recorder's uint16 (Q << 8 | I)."""
    from gpsmi import codes
    rng = np.random.default_rng(seed)
    n = n_ms * cs
    x = np.zeros(n)
    for prn, d in ((P1, 300), (P2, 1200)):
        x += 0.6 * np.roll(np.tile(codes.code_replica(prn, cs).astype(np.float64), n_ms), d)
    z = x + 0.5 * rng.standard_normal(n) + 0.5j * rng.standard_normal(n)
    i8 = np.clip(np.rint(127.5 + 30 * z.real), 0, 255).astype(np.uint16)
    q8 = np.clip(np.rint(127.5 + 30 * z.imag), 0, 255).astype(np.uint16)
    return z.astype(np.complex64), (q8 << 8 | i8).astype(np.uint16)


def _acq(cs, raw_u8):
    from gpsmi.engine import AcqEngine, Config
    e = AcqEngine(Config(code_samples=cs, n_cyc=8), prns=(P1, P2, P3))
    if raw_u8:
        e.set_input_format(True)
    return e


def _run_reused_and_fresh(make, steps):
    """Every step on one handle, in order, and each alone on a handle of its own."""
    reused = make()
    try:
        for k, step in enumerate(steps):
            got = step(reused)
            fresh = make()
            try:
                want = step(fresh)
            finally:
                fresh.close()
            try:
                _same_all(got, want)
            except AssertionError as err:
                raise AssertionError('step %d differs from a fresh handle' % k) from err
    finally:
        reused.close()


@pytest.mark.parametrize('raw_u8', [False, True], ids=['c64', 'u8'])
def test_acq_2048(raw_u8):
    """search (3, 1), (9, 3), (3, 1); search_nc and search_deep with n_seg 2; refine of 1 and of 2
    hits; acq_track of 1 hit; cancel of 1, of 2 and of 1 satellite (the last with the coefficients);
    search (3, 1) again -- all from host memory, so each grows the one input buffer they share.  A
    complex64 cancel works in place in that buffer, a raw one beside it, and the search that follows
    reads the buffer again."""
    from gpsmi.acquisition import open_weak_channels
    from gpsmi.engine import Config
    cs = 2048
    iq = _scene(cs, 70, 1)[1 if raw_u8 else 0]
    f3, f9 = np.array([-1000.0, 0.0, 1000.0]), np.linspace(-2000.0, 2000.0, 9)
    e = _acq(cs, raw_u8)
    try:                                                   # the hits and the state the steps use
        tab = e.search(iq, (P1, P2), [0.0], 1)
        hits = [(P1, 0.0, int(tab[0, 0]['argmax'])), (P2, 0.0, int(tab[0, 1]['argmax']))]
        state = open_weak_channels(e.refine(iq, hits[:1], 40), Config(code_samples=cs, n_cyc=8))
    finally:
        e.close()
    steps = [
        lambda h: h.search(iq, (P1,), f3, 1),
        lambda h: h.search_ex(iq, (P1, P2, P3), f9, 2),
        lambda h: h.search(iq, (P1,), f3, 1),
        lambda h: h.search_noncoherent(iq, (P1,), f3, 1, 2, nbr=True),
        lambda h: h.search_deep(iq, (P1, P2), f3, 2, 2, nbr=True),
        lambda h: h.refine(iq, hits[:1], 40, want_grid=True, want_prompts=True),
        lambda h: h.refine(iq, hits, 40, want_grid=True, want_prompts=True),
        lambda h: h.track_weak(iq, state, 1),
        lambda h: h.cancel(iq, SATS[:1]),
        lambda h: h.cancel(iq, SATS),
        lambda h: h.cancel(iq, SATS[:1], coef=True),
        lambda h: h.search(iq, (P1,), f3, 1),
    ]
    _run_reused_and_fresh(lambda: _acq(cs, raw_u8), steps)


def test_acq_rows_and_collective():
    """search_deep with rows (2 PRNs, 3 bins, n_seg 2) from host memory; collective over those rows
    (2 satellites, a 2 x 2 x 1 grid) without and then with pooling, so the pooled half of the scratch
    appears after the handle sized it without; the deep search again with 1 PRN."""
    from gpsmi._lib import COLLECTIVE_SAT_DTYPE
    from gpsmi.engine import DeviceBuffer
    cs = 2048
    iq = _scene(cs, 70, 1)[0]
    f3 = np.array([-1000.0, 0.0, 1000.0])
    sats = np.zeros(2, dtype=COLLECTIVE_SAT_DTYPE)      # (row, bin_lo, bin_hi, -, lag0, g_e, g_n, g_t)
    sats[0] = (0, 0, 2, 0, 300.0, 0.75, -0.5, 0.0)
    sats[1] = (1, 0, 2, 0, 1200.0, -1.25, 0.5, 0.0)
    grid = dict(n_e=2, n_n=2, n_t=1, e0=-1.0, n0=-1.0, d_e=2.0, d_n=2.0)
    rows = DeviceBuffer(2 * len(f3) * cs * 4)

    def deep(prns):
        def run(h):
            tab = h.search_deep(iq, prns, f3, 2, 2, rows=rows)
            return tab, rows.download(np.float32, len(prns) * len(f3) * cs)
        return run

    try:
        # (the rows of the first step stay in the buffer for the two that follow: the fresh handle of
        # a step writes what the reused one wrote)
        _run_reused_and_fresh(lambda: _acq(cs, False), [
            deep((P1, P2)),
            lambda h: h.collective(rows, sats, dict(grid, pool=1), nsv_rows=2, nbins=3),
            lambda h: h.collective(rows, sats, dict(grid, pool=2), nsv_rows=2, nbins=3),
            deep((P1,)),
        ])
    finally:
        rows.free()


@pytest.mark.parametrize('raw_u8', [False, True], ids=['c64', 'u8'])
def test_acq_host_and_device_input_agree(raw_u8):
    """Every entry point that takes iq from host memory or as a (device pointer, n) pair gives the
    same bytes for both: search, search_noncoherent, search_deep, refine (40 ms, one hit), track_weak
    (one bit) and cancel (one satellite, into a device buffer of its own)."""
    from gpsmi.acquisition import open_weak_channels
    from gpsmi.engine import Config, DeviceBuffer
    cs = 2048
    iq = _scene(cs, 70, 1)[1 if raw_u8 else 0]
    f3 = np.array([-1000.0, 0.0, 1000.0])
    d_iq, d_out = DeviceBuffer(iq.nbytes), DeviceBuffer(iq.size * 8)
    d_iq.upload(iq)
    dev = (d_iq.ptr, iq.size)
    e_host, e_dev = _acq(cs, raw_u8), _acq(cs, raw_u8)
    try:
        tab = e_host.search(iq, (P1,), [0.0], 1)
        hit = [(P1, 0.0, int(tab[0, 0]['argmax']))]
        state = open_weak_channels(e_host.refine(iq, hit, 40), Config(code_samples=cs, n_cyc=8))
        calls = [
            lambda h, x: h.search(x, (P1, P2), f3, 1),
            lambda h, x: h.search_noncoherent(x, (P1, P2), f3, 1, 2),
            lambda h, x: h.search_deep(x, (P1, P2), f3, 2, 2),
            lambda h, x: h.refine(x, hit, 40, want_grid=True, want_prompts=True),
            lambda h, x: h.track_weak(x, state, 1),
        ]
        for k, call in enumerate(calls):
            try:
                _same_all(call(e_host, iq), call(e_dev, dev))
            except AssertionError as err:
                raise AssertionError('call %d differs between host and device input' % k) from err
        out, rec = e_host.cancel(iq, SATS[:1])
        _, rec_dev = e_dev.cancel(dev, SATS[:1], out=d_out.ptr)
        _same_all((out, rec), (d_out.download(np.complex64, iq.size), rec_dev))
    finally:
        e_host.close()
        e_dev.close()
        d_iq.free()
        d_out.free()


def test_acq_16368():
    """search (2, 1), search_nc (2, 2) with n_seg 2, search (3, 1): the cell tables the coherent and
    the non-coherent search share, with and without the magnitude plane beside them."""
    cs = 16368
    iq = _scene(cs, 2, 2)[0]
    steps = [
        lambda h: h.search(iq, (P1,), [-500.0, 0.0], 1),
        lambda h: h.search_noncoherent(iq, (P1, P2), [-500.0, 0.0], 1, 2, nbr=True),
        lambda h: h.search_ex(iq, (P1,), [-500.0, 0.0, 500.0], 1),
    ]
    _run_reused_and_fresh(lambda: _acq(cs, False), steps)


def test_trk_2048():
    """replay of 1, 4 and 1 blocks on a handle of 2 channels (the job tables regrow past max_ch and
    are then larger than needed), then one closed-loop block."""
    from gpsmi.engine import Config, DeviceBuffer, TrkEngine
    cfg = Config(code_samples=2048, n_cyc=8)
    nb_max = 4
    iq = _scene(2048, nb_max * cfg.n_cyc, 3)[0]
    chans = ((P1, 0.0, 300), (P2, 0.0, 1200))

    def make():
        t = TrkEngine(cfg, max_ch=2, prns=(P1, P2))
        for ch, (prn, f, d) in enumerate(chans):
            t.open(ch, prn, f, d)
        return t

    t = make()
    try:
        row = np.array([t.get_state(ch) for ch in range(2)])
    finally:
        t.close()
    table = np.ascontiguousarray(np.broadcast_to(row, (nb_max, 2)))
    d_iq = DeviceBuffer(iq.nbytes)
    d_iq.upload(iq)

    def replay(nb):
        def run(h):
            out, st = h.replay(d_iq.at(0), nb, table[:nb]), h.replay_states(nb)
            # a state's drift list is defined up to df_len: the replay writes that much of it into
            # memory it does not clear (test_gpu_trk.py compares it the same way)
            keep = np.arange(st['df'].shape[-1]) < st['df_len'][..., None]
            st['df'] = np.where(keep, st['df'], 0)
            return out, st
        return run

    def process(h):
        out = h.process(iq[:cfg.ngps])
        return out, np.array([h.get_state(ch) for ch in range(2)])

    try:
        _run_reused_and_fresh(make, [replay(1), replay(4), replay(1), process])
    finally:
        d_iq.free()


def _blocks(n, nb, raw_u8, seed):
    """nb blocks of n samples of noise with a few strong pulses and a tone (something to blank and to
    excise), in either input format."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(nb * n) + 1j * rng.standard_normal(nb * n)
    z += 2.0 * np.exp(2j * np.pi * 0.123 * np.arange(nb * n))
    z[::701] *= 6.0
    if not raw_u8:
        return z.astype(np.complex64).reshape(nb, n)
    i8 = np.clip(np.rint(127.5 + 12 * z.real), 0, 255).astype(np.uint16)
    q8 = np.clip(np.rint(127.5 + 12 * z.imag), 0, 255).astype(np.uint16)
    return (q8 << 8 | i8).astype(np.uint16).reshape(nb, n)


def _filter_steps(x, results):
    def step(nb):
        def run(h):
            h.reset()
            out = h.apply(x[:nb])
            return (out,) + tuple(getattr(h, r) for r in results)
        return run
    return [step(1), step(3), step(1)]


@pytest.mark.parametrize('raw_u8', [False, True], ids=['c64', 'u8'])
def test_pb(raw_u8):
    """pulse blanking at its smallest block, 2048 samples: 1, 3, 1 blocks from host memory."""
    from gpsmi.blanking import PulseBlanker
    from gpsmi.engine import Config
    cfg = Config(code_samples=2048, n_cyc=1)
    x = _blocks(cfg.ngps, 3, raw_u8, 4)
    _run_reused_and_fresh(lambda: PulseBlanker(cfg, thresh_db=6.0, raw_u8=raw_u8),
                          _filter_steps(x, ('last_counts', 'last_floors', 'last_masks')))


@pytest.mark.parametrize('raw_u8', [False, True], ids=['c64', 'u8'])
def test_ifx(raw_u8):
    """excision at its smallest block, 4096 samples: 1, 3, 1 blocks from host memory."""
    from gpsmi.engine import Config
    from gpsmi.excision import Excision
    cfg = Config(code_samples=2048, n_cyc=2)
    x = _blocks(cfg.ngps, 3, raw_u8, 5)
    _run_reused_and_fresh(lambda: Excision(cfg, thresh_db=3.0, raw_u8=raw_u8),
                          _filter_steps(x, ('last_counts', 'last_masks')))


@pytest.mark.parametrize('fmt', ['c64', 'u8iq'])
def test_fe(fmt):
    """the front end (2.0 -> 2.048 MHz): pieces of 2000, 6000 and 2000 input samples, reset between
    (the stage has no block size of its own: a piece is one millisecond of input)."""
    from gpsmi.engine import Config
    from gpsmi.frontend import FrontEnd
    cfg = Config(code_samples=2048, n_cyc=8)
    x = _blocks(2000, 3, fmt == 'u8iq', 6)

    def step(nb):
        def run(h):
            h.reset()
            return h.push(x[:nb])
        return run

    _run_reused_and_fresh(lambda: FrontEnd(cfg, 2_000_000, fmt, max_out=8192), [step(1), step(3), step(1)])
