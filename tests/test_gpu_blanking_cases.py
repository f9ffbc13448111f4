"""The blanking kernels (csrc/gpsmi_pb.hip) on the pinned cases of tests/pb_cases.py, bit for bit
against the numpy restatement (tests/pb_ref.py): outputs, counts, floors and masks, at block lengths
with partial word groups and partial slices, guards up to 1024, detections at the limit of the guard
comparison, powers that only the last pass of the select tells apart, and the carry in every way it
travels."""
import os

import numpy as np
import pytest

import pb_cases as PC
import pb_ref as R

pytestmark = pytest.mark.gpu


def _blanker(n, thresh_db, pre, post, max_frac, raw_u8=False):
    from gpsmi.blanking import PulseBlanker
    from gpsmi.engine import Config
    pb = PulseBlanker(Config(code_samples=n, n_cyc=1), thresh_db, pre, post, max_frac, raw_u8)
    assert pb.n == n
    return pb


def _same(pb, want, y, what=None):
    """The call's output and per-block results equal the restatement's (y, counts, floors, masks)."""
    y_r, c_r, f_r, m_r = want
    assert np.array_equal(pb.last_counts, c_r), (what, pb.last_counts, c_r)
    assert pb.last_floors.tobytes() == f_r.tobytes(), (what, pb.last_floors, f_r)
    assert pb.last_masks.tobytes() == m_r.tobytes(), what
    assert np.asarray(y).reshape(y_r.shape).tobytes() == y_r.tobytes(), what


def _ref(xs, n, thresh_db, pre, post, max_frac):
    return R.BlankerRef(n, thresh_db, pre, post, max_frac).run(xs)


@pytest.mark.parametrize('n, guard', PC.GEOMETRY, ids=lambda v: str(v).replace(' ', ''))
def test_geometry_matrix(n, guard):
    pre, post = guard
    blocks, _, labels = PC.geometry_blocks(n, pre, post)
    args = (n, PC.GEO_THRESH_DB, pre, post, PC.GEO_MAX_FRAC)
    pb = _blanker(*args)
    for k in range(0, len(blocks), 3):
        what = labels[k:k + 3]
        triple = blocks[k:k + 3]
        wide = PC.spread16(triple, 4000 + k)
        want3, want16 = _ref(triple, *args), _ref(wide, *args)
        for i, carry in PC.carries_of(what, post):      # the carries of the triple arrive within the call
            assert i < 2 and want3[1][i + 1] == carry and want16[1][(0, 7, 15)[i] + 1] == carry, what
        pb.reset()
        _same(pb, want3, pb.apply(triple), (what, 'small slices'))
        pb.reset()
        _same(pb, want16, pb.apply(wide), (what, 'large slices'))
    pb.close()


@pytest.mark.parametrize('n', PC.RAW_LENGTHS)
def test_raw_input(n):
    from gpsmi import synth
    for spiked, thresh_db, guards in ((True, 10.0, PC.RAW_GUARDS), (False, 0.0, PC.RAW_TIE_GUARDS)):
        raw = PC.raw_blocks(n, spiked)
        x = synth.raw_to_c64(raw)
        for pre, post in guards:
            args = (n, thresh_db, pre, post, 1.0)
            want = _ref(x, *args)
            pb_u8, pb_c = _blanker(*args, raw_u8=True), _blanker(*args)
            _same(pb_u8, want, pb_u8.apply(raw), (spiked, pre, post, 'u8'))
            _same(pb_c, want, pb_c.apply(x), (spiked, pre, post, 'complex64'))
            pb_u8.close()
            pb_c.close()


@pytest.mark.parametrize('thresh_db', PC.SELECT_THRESH_DB)
def test_select(thresh_db):
    """Powers a few ulp apart, two values, NaN / Inf, subnormal powers: the floors first,
    block by block, then everything."""
    blocks = PC.select_blocks()
    args = (PC.SELECT_N, thresh_db) + PC.SELECT_GUARD + (1.0,)
    want = _ref(blocks, *args)
    pb = _blanker(*args)
    y = pb.apply(blocks)
    for b, label in enumerate(PC.SELECT_LABELS):
        assert pb.last_floors[b:b + 1].tobytes() == want[2][b:b + 1].tobytes(), \
            (label, pb.last_floors[b], want[2][b])
        assert pb.last_counts[b] == want[1][b], (label, pb.last_counts[b], want[1][b])
    _same(pb, want, y)
    pb.close()


def test_carry_out_of_a_block_that_passed_through():
    c = PC.CARRY
    args = (c['n'], c['thresh_db'], c['pre'], c['post'], c['max_frac'])
    blocks = PC.carry_blocks()
    want = _ref(blocks, *args)
    assert want[1].tolist() == [-1, c['post']]
    pb = _blanker(*args)
    _same(pb, want, pb.apply(blocks), 'one call')
    pb.reset()
    for b in (0, 1):                                    # block 1 in a call of its own
        _same(pb, tuple(v[b:b + 1] for v in want), pb.apply(blocks[b]), f'call {b}')
    pb.reset()
    pb.apply(blocks[0])
    pb.reset()                                          # no carry survives a reset
    alone = _ref(blocks[1:], *args)
    assert alone[1].tolist() == [0]
    _same(pb, alone, pb.apply(blocks[1]), 'after reset')
    pb.close()


def test_chunking():
    c = PC.CHUNK
    args = (c['n'], c['thresh_db'], c['pre'], c['post'], c['max_frac'])
    blocks = PC.chunk_blocks()
    os.environ['GPSMI_PB_CHUNK_MIB'] = '1'
    try:
        chunked = _blanker(*args)
    finally:
        del os.environ['GPSMI_PB_CHUNK_MIB']
    whole = _blanker(*args)
    want = _ref(blocks, *args)
    y_c, y_w = chunked.apply(blocks), whole.apply(blocks)
    _same(chunked, want, y_c, 'chunked')
    _same(whole, want, y_w, 'one chunk')
    assert y_c.tobytes() == y_w.tobytes()
    for k in ('last_counts', 'last_floors', 'last_masks'):
        assert getattr(chunked, k).tobytes() == getattr(whole, k).tobytes(), k
    chunked.close()
    whole.close()
