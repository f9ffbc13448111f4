"""Size-independent properties at BASELINE's full tracking size (configs[2]: 1024 blocks x
65536 samples x 12 channels, 512 MiB resident) -- far beyond what the oracle can check
sample by sample:

* linearity: the same batch with the IQ doubled gives exactly doubled dumps / taps /
  statistics (every operation on the data path is linear, and x2 is exact in float32)
  and unchanged argmax, DELAY, code phase, normMaxCorr, PLL outputs;
* position independence: the batch repeats every 16 blocks with identical state rows,
  so block i and block i+16 must agree bytewise although they run in different
  workgroups, on different XCDs and with a different wave <-> quarter rotation.

The same two properties at configs[4] (512 blocks x 130944 samples x 12 channels,
CODE_SAMPLES = 16368, N_CYC = 8: the general path's fold, pfa_corr and span8 grids), and
replays of the recorded fixture trajectories (ref_hirate; ref_ncyc16 / ref_ncyc8 at 512 MiB)
tiled over the whole batch, every tile bytewise the closed loop's outputs.  One large buffer
is live at a time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NB, NCH, NGPS, PERIOD = 1024, 12, 65536, 16


def test_linearity_and_position_independence_at_full_size():
    _linearity_and_position_independence(None, NB, NGPS)


def test_configs4_linearity_and_position_independence_at_full_size():
    """configs[4]: the general path (trk_fold_general_kernel, pfa_corr_kernel, trk_span8_kernel)."""
    from gpsmi.engine import Config
    _linearity_and_position_independence(Config(code_samples=16368, n_cyc=8), 512, 16368 * 8)


def _linearity_and_position_independence(cfg, nb, ngps):
    from gpsmi import engine as E
    rng = np.random.default_rng(99)
    trk = E.TrkEngine(cfg, max_ch=NCH)
    cs = trk.cfg.code_samples
    assert nb % PERIOD == 0 and trk.cfg.ngps == ngps
    chunk = (rng.standard_normal((PERIOD, ngps, 2)) * 0.25).astype(np.float32)
    for c in range(NCH):
        trk.open(c, 2 + c, -4000.0 + 700.0 * c, (1137 * c + 11) % cs)
    st = np.zeros((nb, NCH), dtype=E.STATE_DTYPE)
    for c in range(NCH):
        st[:, c] = trk.get_state(c)
    ph = rng.uniform(0, 6.28, (PERIOD, NCH)).astype(np.float32)
    st['phase'] = np.tile(ph, (nb // PERIOD, 1))                 # state rows repeat too
    dly = np.broadcast_to(st['delay'][0], (nb, NCH)).copy()
    buf = E.DeviceBuffer(nb * ngps * 8)
    outs = []
    for scale in (1.0, 2.0):
        data = chunk * np.float32(scale)
        for i in range(0, nb, PERIOD):
            buf.upload(data, i * ngps * 8)
        outs.append(trk.replay(buf.ptr, nb, st, dly).copy())
    buf.free()
    trk.close()
    a, b = outs
    # ---- linearity
    for k in ('mx', 'delay', 'delay_used', 'n_dumps', 'first_len', 'nps', 'phase_locked'):
        assert np.array_equal(a[k], b[k]), k
    for k in ('dumps', 'epl', 'corr_mean', 'corr_std', 'std_dev'):
        assert np.array_equal(2 * a[k], b[k]), k
    for k in ('norm_max_corr', 'code_phase', 'amplitude', 'df', 'phase_shift', 'freq', 'phase'):
        assert np.array_equal(a[k], b[k]), k
    assert np.abs(a['dumps']).max() > 0 and np.isfinite(a['dumps']).all()
    # ---- position independence
    ref = a[:PERIOD]
    for i in range(PERIOD, nb, PERIOD):
        assert a[i:i + PERIOD].tobytes() == ref.tobytes(), i


def _tiled_replay_equals_closed_loop(eng, outs, states, blocks, nb_full):
    """Replay of nb_full blocks in one launch: the recorded blocks, their start-of-block state
    rows and DELAYs repeated tile after tile (the last tile cut short).  Every tile must equal
    the closed loop's outputs bytewise."""
    from gpsmi.engine import DeviceBuffer
    nb = len(blocks)
    assert outs.shape[0] == nb and nb_full > nb
    rows = np.arange(nb_full) % nb
    tile = np.stack(blocks)
    buf = DeviceBuffer(nb_full * tile[0].nbytes)
    try:
        for t0 in range(0, nb_full, nb):
            buf.upload(tile[:min(nb, nb_full - t0)], t0 * tile[0].nbytes)
        rep = eng.replay(buf.ptr, nb_full, states[rows], outs['delay_used'][rows])
    finally:
        buf.free()
    assert rep.shape == (nb_full, outs.shape[1])
    for t0 in range(0, nb_full, nb):
        n = min(nb, nb_full - t0)
        assert rep[t0:t0 + n].tobytes() == outs[:n].tobytes(), t0


def test_configs4_replay_of_the_hirate_trajectory_at_full_size(golden_hirate):
    """configs[4] on real signal: the closed loop over ref_hirate's 40 blocks, then those blocks
    tiled over 512 (12 full tiles + 32) in one replay."""
    from gpsmi.engine import Config
    from test_gpu_trk import _run_closed_loop
    eng, outs, states, blocks = _run_closed_loop(golden_hirate, 'hirate',
                                                 Config(code_samples=16368, n_cyc=8))
    try:
        assert eng.cfg.ngps == 130944
        _tiled_replay_equals_closed_loop(eng, outs, states, blocks, 512)
    finally:
        eng.close()


@pytest.mark.parametrize('cfg', ['ncyc16', 'ncyc8'])
def test_other_block_length_replay_of_the_fixture_trajectory_at_512_mib(cfg):
    """N_CYC = 16 / 8 at CODE_SAMPLES = 2048 at the bench's size (512 MiB of complex64: 2048 /
    4096 blocks): the fixture trajectory tiled, complex64 and raw uint16 blocks alike."""
    from test_gpu_trk import _closed_loop_ncyc
    from test_oracle import ncyc_scene
    g, (eng, outs, states, blocks) = _closed_loop_ncyc(cfg)
    try:
        nb_full = (512 << 20) // (eng.cfg.ngps * 8)
        assert nb_full == {'ncyc16': 2048, 'ncyc8': 4096}[cfg]
        _tiled_replay_equals_closed_loop(eng, outs, states, blocks, nb_full)
        sc = ncyc_scene(cfg)
        raw = [sc.block_raw(5 + i) for i in range(len(blocks))]
        eng.set_input_format(True)
        _tiled_replay_equals_closed_loop(eng, outs, states, raw, nb_full)
    finally:
        eng.close()
