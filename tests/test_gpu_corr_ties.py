"""Ties through the library: a correlation whose 2048 magnitudes are all equal must report lag 0,
in every form of the code-phase correlation kernel and in the acquisition search.

All-zero complex64 IQ makes every magnitude +0: the first index of the maximum is lag 0, peak,
neighbours, mean and standard deviation are 0, (0 - 0) / 0 is no number above CORR_MIN, so the
block reports delay -1.  The raw uint16 format cannot hold a zero sample (a byte b decodes to
b / 127.5 - 1, which is never 0), so its leg runs the nearest thing it can say: one constant raw
block and its complex64 decode, whose records must be the same bytes under every CG and in both
formats."""
import numpy as np
import pytest

CORR_MIN = 8.0
BIG = 1 << 24
# (CG, how it is forced): as tests/test_gpu_trk_corr.py forces it
CG_SETTINGS = (
    (1, (('corr_small2', BIG), ('corr_small1', BIG))),
    (2, (('corr_small1', 0), ('corr_small2', BIG))),
    (2, (('corr_small1', 0), ('corr_small2', 0), ('corr_cg', 2))),
    (4, (('corr_small1', 0), ('corr_small2', 0), ('corr_cg', 4))),
    (6, (('corr_small1', 0), ('corr_small2', 0), ('corr_cg', 6))),
)
FIELDS = ('mx', 'epl', 'corr_mean', 'corr_std', 'norm_max_corr', 'delay', 'code_phase', 'delay_used')
NCH = 13
N_CYC = 32


def _table():
    from gpsmi.engine import STATE_DTYPE, TrkEngine
    eng = TrkEngine(max_ch=1)
    eng.open(0, 3, 0.0, 0)
    row = eng.get_state(0).copy()
    eng.close()
    table = np.empty((1, NCH), dtype=STATE_DTYPE)
    table[...] = row
    for c in range(NCH):
        table[0, c]['prn'] = 1 + 2 * c
        table[0, c]['freq'] = np.float32(-5000.0 + 800.0 * c)
        table[0, c]['omega0'] = np.float32(0)
        table[0, c]['phase'] = np.float32(0.4 * c)
        table[0, c]['delay'] = (0, 2047, 100 * c)[min(c % 4, 2)]
    return table, np.full((1, NCH), -1, dtype=np.int32)


def _replay_all(inputs):
    """{(cg index, format): records [1, NCH]} of one block given as {'c64': ..., 'u8': ...}."""
    from gpsmi.engine import Config, DeviceBuffer, TrkEngine
    table, forced = _table()
    eng = TrkEngine(Config(n_cyc=N_CYC, corr_avg=8, corr_min=CORR_MIN), max_ch=NCH)
    bufs, out = {}, {}
    try:
        for fmt, block in inputs.items():
            bufs[fmt] = DeviceBuffer(block.nbytes)
            bufs[fmt].upload(block)
        for i, (cg, settings) in enumerate(CG_SETTINGS):
            for key, value in settings:
                eng.set_option(key, value)
            for fmt in inputs:
                eng.set_input_format(fmt == 'u8')
                out[i, fmt] = eng.replay(bufs[fmt].ptr, 1, table, forced).copy()
    finally:
        for b in bufs.values():
            b.free()
        eng.close()
    return out


def _bytes(rec):
    return b''.join(np.ascontiguousarray(rec[k]).tobytes() for k in FIELDS)


@pytest.mark.gpu
def test_zero_block_reports_lag_0_under_every_cg():
    out = _replay_all({'c64': np.zeros(N_CYC * 2048, dtype=np.complex64)})
    assert len(out) == len(CG_SETTINGS)
    first = None
    for key, rec in out.items():
        assert rec.shape == (1, NCH)
        assert np.array_equal(rec['mx'], np.zeros((1, NCH), np.int32)), (key, rec['mx'])
        assert rec['epl'].tobytes() == np.zeros((1, NCH, 3), np.float32).tobytes(), (key, rec['epl'])
        assert rec['corr_mean'].tobytes() == np.zeros((1, NCH), np.float32).tobytes(), key
        assert rec['corr_std'].tobytes() == np.zeros((1, NCH), np.float32).tobytes(), key
        assert np.array_equal(rec['delay'], np.full((1, NCH), -1, np.int32)), (key, rec['delay'])
        first = first if first is not None else _bytes(rec)
        assert _bytes(rec) == first, key


@pytest.mark.gpu
def test_constant_raw_block_same_bytes_across_cg_and_format():
    from gpsmi import synth
    raw = np.full(N_CYC * 2048, 0x8080, dtype=np.uint16)
    c64 = synth.raw_to_c64(raw)
    assert c64.dtype == np.complex64 and np.all(c64 == c64[0]) and c64[0] != 0
    out = _replay_all({'c64': c64, 'u8': raw})
    assert len(out) == 2 * len(CG_SETTINGS)
    first = _bytes(out[0, 'c64'])
    for key, rec in out.items():
        assert _bytes(rec) == first, key


@pytest.mark.gpu
def test_zero_millisecond_search_reports_lag_0():
    """The shape of the search a replay step runs beside the correlation, cut down: 2 SVs x 3 bins
    on 1 ms of zeros."""
    from gpsmi.engine import AcqEngine
    eng = AcqEngine()
    try:
        tab, nbr = eng.search_ex(np.zeros(2048, dtype=np.complex64), [1, 2], [-200.0, 0.0, 200.0], 1)
        plain = eng.search(np.zeros(2048, dtype=np.complex64), [1, 2], [-200.0, 0.0, 200.0], 1)
    finally:
        eng.close()
    assert tab.shape == (3, 2) and nbr.shape == (3, 2, 2)
    assert np.array_equal(tab['argmax'], np.zeros((3, 2), np.int32)), tab['argmax']
    for k in ('peak', 'mean', 'std'):
        assert tab[k].tobytes() == np.zeros((3, 2), np.float32).tobytes(), (k, tab[k])
    assert nbr.tobytes() == np.zeros((3, 2, 2), np.float32).tobytes(), nbr
    assert plain.tobytes() == tab.tobytes()
