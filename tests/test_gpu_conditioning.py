"""conditioning.Conditioner (the chain a Receiver runs its blocks through) and ingest.open_blocks /
take against what they replace: the stages applied one after the other through their host entry,
one batched call over all blocks, and the reader loops written out.

Blocks of 4096 samples: the smallest the excision takes, and two slices per block for the blanker,
so its halo is on the path.  Three consecutive blocks of noise (sigma 0.03) under a tone 25 dB up at
bin 300.5, with 8-sample bursts 20 dB up at samples 4093 (across the end of block 0), 6096 and 9192.
With tests/ifx_ref.ExcisionRef and tests/pb_ref.BlankerRef the scene gives, on the CPU: excision
counts 186 / 39 / 34 and, behind it, blanking counts 34 / 202 / 192 for complex64; 180 / 39 / 34 and
39 / 205 / 183 for u8; the blanker's carry is 2 into blocks 1 and 2 in both (the excision leaves the
tone's step at a block's flat-windowed end).  A blanker alone finds nothing in this scene -- the tone
raises every sample's power, which is why the chain excises first -- so the blank-only chain also runs
on the scene without the tone: counts 15 / 39 / 17 for complex64, 35 / 59 / 12 for u8, carry 2 into
block 1."""
import numpy as np
import pytest

import ifx_ref

pytestmark = pytest.mark.gpu

N, NB, SIGMA, SEED = 4096, 3, 0.03, 7
BURSTS = (4093, 6096, 9192)
_CACHE = {}


def _cfg(n_cyc=2):
    from gpsmi.engine import Config
    return Config(code_samples=2048, n_cyc=n_cyc)


def _scene(fmt, tone=True):
    """[NB, N] complex64, or the recorder's uint16 of the same samples (fmt 'u8')."""
    key = (fmt, tone)
    if key not in _CACHE:
        rng = np.random.default_rng(SEED)
        x = (SIGMA / np.sqrt(2.0)) * (rng.standard_normal(NB * N) + 1j * rng.standard_normal(NB * N))
        if tone:
            k = np.arange(NB * N, dtype=np.float64)
            x = x + SIGMA * 10.0 ** (25.0 / 20.0) * np.exp(1j * (2.0 * np.pi * ((300.5 * k) % 2048) / 2048 + 0.3))
        for s in BURSTS:
            x[s:s + 8] += SIGMA * 10.0 * (rng.standard_normal(8) + 1j * rng.standard_normal(8)) / np.sqrt(2.0)
        x = x.reshape(NB, N)
        _CACHE[key] = ifx_ref.quantise(x) if fmt == 'u8' else x.astype(np.complex64)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _stages(excise, blank, raw_u8):
    from gpsmi.blanking import PulseBlanker
    from gpsmi.excision import Excision
    out = [Excision(_cfg(), raw_u8=raw_u8)] if excise else []
    if blank:
        out.append(PulseBlanker(_cfg(), raw_u8=raw_u8 and not excise))
    return out


def _check_chain(xs, excise, blank, raw_u8):
    """-> (excision counts, blanking counts, blanking masks) of the chain, block by block."""
    from gpsmi.conditioning import Conditioner
    cond = Conditioner(_cfg(), raw_u8, excise=excise, blank=blank)
    assert cond.out_raw_u8 is False and bool(cond)
    got, e_counts, b_counts, b_masks = [], [], [], []
    for x in xs:
        y = cond.apply(x)
        assert y is cond.last and y.dtype == np.complex64
        got.append(y.copy())
        if excise:
            e_counts.append(int(cond.excision.last_counts[0]))
        if blank:
            b_counts.append(int(cond.blanker.last_counts[0]))
            b_masks.append(cond.blanker.last_masks[0].copy())
    cond.close()
    got = np.stack(got)

    one_by_one = _stages(excise, blank, raw_u8)
    for b, x in enumerate(xs):
        for st in one_by_one:
            x = st.apply(x)
        assert x.tobytes() == got[b].tobytes(), f'block {b}: not the stages applied one after the other'
    batched = _stages(excise, blank, raw_u8)
    y = xs
    for st in batched:
        y = st.apply(y)
    assert y.tobytes() == got.tobytes(), 'not the stages applied to all blocks at once'
    for st, k in zip(batched, [e_counts] * excise + [b_counts] * blank):
        assert st.last_counts.tolist() == k
    for st in one_by_one + batched:
        st.close()
    print('excision counts', e_counts, 'blanking counts', b_counts)
    return e_counts, b_counts, b_masks


@pytest.mark.parametrize('fmt', ['c64', 'u8'])
@pytest.mark.parametrize('mode', ['off', 'excise', 'blank', 'both'])
def test_chain_equals_its_stages_block_by_block_and_batched(mode, fmt):
    from gpsmi.conditioning import Conditioner
    raw_u8, xs = fmt == 'u8', _scene(fmt)
    if mode == 'off':
        cond = Conditioner(_cfg(), raw_u8)
        assert not cond and cond.out_raw_u8 is raw_u8 and cond.excision is None and cond.blanker is None
        for x in xs:
            assert cond.apply(x) is x and cond.last is x
        cond.close()
        return
    excise, blank = mode in ('excise', 'both'), mode in ('blank', 'both')
    e_counts, b_counts, b_masks = _check_chain(xs, excise, blank, raw_u8)
    assert all(c > 0 for c in e_counts)                 # (neither -1 nor nothing to do)
    if mode == 'both':
        assert all(c > 0 for c in b_counts)
        post = 2                                        # blanking.default_guard(2048)
        for b in (1, 2):                                # the carry crossed both block boundaries
            assert int(b_masks[b][0]) & (1 << post) - 1 == (1 << post) - 1, b
    if mode == 'blank':
        assert all(c == 0 for c in b_counts)            # (the tone hides the bursts: see the docstring)
        _, b_counts, b_masks = _check_chain(_scene(fmt, tone=False), False, True, raw_u8)
        assert all(c > 0 for c in b_counts)
        assert int(b_masks[1][0]) & 3 == 3


def test_close_leaves_a_borrowed_stage_open_and_closes_its_own():
    from gpsmi.conditioning import Conditioner
    from gpsmi.excision import Excision
    xs = _scene('c64')
    mine = Excision(_cfg())
    cond = Conditioner(_cfg(), False, excise=mine, blank=True)
    assert cond.excision is mine
    theirs = cond.blanker
    cond.apply(xs[0])
    cond.close()
    assert theirs.h is None and mine.h is not None
    mine.reset()
    assert mine.apply(xs[0]).shape == (N,) and mine.last_counts[0] > 0
    mine.close()


def test_a_stage_that_does_not_match_is_refused():
    from gpsmi.blanking import PulseBlanker
    from gpsmi.conditioning import Conditioner
    from gpsmi.excision import Excision
    ex_u8, ex_long, pb_u8 = Excision(_cfg(), raw_u8=True), Excision(_cfg(4)), PulseBlanker(_cfg(), raw_u8=True)
    with pytest.raises(ValueError, match='the Excision does not match raw_u8 / the block length'):
        Conditioner(_cfg(), False, excise=ex_u8)
    with pytest.raises(ValueError, match='the Excision does not match raw_u8 / the block length'):
        Conditioner(_cfg(), False, excise=ex_long)
    with pytest.raises(ValueError, match='the PulseBlanker does not match raw_u8 / the block length'):
        Conditioner(_cfg(), False, blank=pb_u8)
    with pytest.raises(ValueError, match='the PulseBlanker does not match raw_u8 / the block length'):
        Conditioner(_cfg(), True, excise=ex_u8, blank=pb_u8)     # (behind an excision: complex64)
    cond = Conditioner(_cfg(), True, blank=pb_u8)
    assert cond.blanker is pb_u8
    cond.close()
    for st in (ex_u8, ex_long, pb_u8):
        st.close()


def test_open_blocks_and_take_read_what_the_reader_loops_read(tmp_path):
    from gpsmi import ingest
    from gpsmi.conditioning import Conditioner
    from gpsmi.frontend import FrontEnd
    cfg = _cfg()
    raw = str(tmp_path / 'raw.bin')
    u8 = _scene('u8')
    np.concatenate([u8.reshape(-1), u8[0, :100]]).tofile(raw)         # (a short last block)
    ref = list(ingest.read_raw_blocks(raw, N, 1))
    assert len(ref) == 2
    with ingest.open_blocks(raw, cfg, start_stream=1) as (blocks, raw_u8):
        assert raw_u8 is True
        got, have = ingest.take(blocks, N + 1)
    assert have == 2 * N and np.array_equal(np.stack(got), np.stack(ref))
    with ingest.open_blocks(raw, cfg, start_stream=2) as (blocks, _):
        got, have = ingest.take(blocks, N + 1)                        # (the stream ends first)
    assert have == N and np.array_equal(got[0], u8[2])

    # an sc16 recording at 4 Msps: some six blocks at the engine's rate; both stages behind it
    frontend = {'fs_in': 4000000, 'fmt': 'sc16'}
    rec = str(tmp_path / 'sc16.bin')
    x = np.resize(_scene('c64').reshape(-1), 50000)
    iq = np.empty(2 * len(x), dtype=np.int16)
    iq[0::2], iq[1::2] = np.rint(x.real * 30000), np.rint(x.imag * 30000)
    iq.tofile(rec)
    fe = FrontEnd(cfg, **frontend)
    ref = [np.array(b) for k, b in enumerate(ingest.read_frontend_blocks(rec, fe)) if k >= 1]
    fe.close()
    assert len(ref) >= 4 and any(not np.array_equal(ref[0], r) for r in ref[1:])
    with ingest.open_blocks(rec, cfg, start_stream=1, frontend=frontend) as (blocks, raw_u8):
        assert raw_u8 is False
        got, have = ingest.take(blocks, 2 * N + 1)
        rest = [np.array(b) for b in blocks]
    assert have == 3 * N and np.array_equal(np.stack(got + rest), np.stack(ref))
    cond, chain = Conditioner(cfg, False, excise=True, blank=True), Conditioner(cfg, False, excise=True, blank=True)
    with ingest.open_blocks(rec, cfg, start_stream=1, frontend=frontend) as (blocks, _):
        got, have = ingest.take(blocks, 3 * N, cond)
    assert have == 3 * N
    for g, r in zip(got, ref):
        assert g.tobytes() == chain.apply(r).tobytes()
    assert not np.array_equal(got[0], ref[0])
    cond.close()
    chain.close()
