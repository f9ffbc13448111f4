"""The pinned blanking cases without a GPU (tests/pb_cases.py): the numpy restatement the kernels are
held to (tests/pb_ref.py) equals an independent brute-force restatement of the contract on every
case, and the cases are what they are meant to be: the detections are the planted spikes, nothing
passes through in the geometry matrix, the spaced pairs sit at the limit of the guard comparison."""
import numpy as np
import pytest

import ifx_ref
import pb_cases as PC
import pb_ref as R


def _same_as_brute(blocks, thresh_db, pre, post, max_frac):
    """BlankerRef.run == brute_run: outputs, counts, floors (bytes) and masks -> the reference's results
    and the final carry."""
    blocks = np.asarray(blocks)
    ref = R.BlankerRef(blocks.shape[1], thresh_db, pre, post, max_frac)
    y, c, f, m = ref.run(blocks)
    y_b, c_b, f_b, b_b, carry = PC.brute_run(blocks, thresh_db, pre, post, max_frac)
    assert np.array_equal(c, c_b), (c, c_b)
    assert f.tobytes() == f_b.tobytes()
    assert np.array_equal(m, np.stack([R.mask_words(b) for b in b_b]))
    assert y.tobytes() == y_b.tobytes()
    assert ref.carry == carry
    return y, c, f, b_b


def test_lengths_are_what_they_are_there_for():
    for n, (words, _) in PC.LENGTHS.items():
        assert n % 32 == 0 and n // 32 == words and n >= 2048
    assert [w % 4 for w, _ in PC.LENGTHS.values()] == [0, 1, 1, 1]
    assert 4128 - 2 * 2048 == 32 and 8192 < 10272 < 2 * 8192 and 10272 % 2048 == 32
    assert PC.WIDE_N // 32 - 3 * 256 == 1 and PC.WIDE_GUARD == (1024, 1024)       # a middle slice with both halos


@pytest.mark.parametrize('n, guard', PC.GEOMETRY, ids=lambda v: str(v).replace(' ', ''))
def test_geometry_matrix(n, guard):
    pre, post = guard
    blocks, planted, labels = PC.geometry_blocks(n, pre, post)
    assert len(blocks) % 3 == 0
    y, counts, floors, blank = _same_as_brute(blocks, PC.GEO_THRESH_DB, pre, post, PC.GEO_MAX_FRAC)
    assert (counts >= 0).all()                          # nothing passes through
    names = set(labels)
    assert {'first', 'words', 'last'} <= names
    for k in (0, 1, 2):                                 # (a pair that does not fit the block is left out)
        assert (f'pair{k}' in names) == (PC.PAIR_AT + pre + post + k < n)
    assert ('slice2048' in names) == (n > 2048) and ('slice8192' in names) == (n > 8192)
    assert ('carry1' in names) == (post > 0)
    for b, label in enumerate(labels):                  # no carry is cut off by the end of a triple
        if label.endswith('+clean'):
            assert b % 3 != 0 and labels[b - 1] == label[:-len('+clean')]
        if label in ('carry1', 'carry0', 'last'):
            assert b % 3 != 2 and labels[b + 1] == label + '+clean'
    for b, (x, spikes, label) in enumerate(zip(blocks, planted, labels)):
        p = R.power(x)
        T = np.float32(floors[b] * R.f_of(PC.GEO_THRESH_DB))
        assert np.flatnonzero(p > T).tolist() == sorted(spikes), label      # the detections: the planted set
        follows = label.endswith('+clean')
        if follows:                                     # (only the carry of the block before)
            want = {'carry1+clean': 1, 'carry0+clean': 0, 'last+clean': post}[label]
            assert counts[b] == want and blank[b][:want].all() and not blank[b][want:].any(), label
        elif spikes:
            assert counts[b] >= len(spikes) and blank[b][spikes].all(), label
        else:
            assert label == 'pad'
        if label.startswith('pair'):
            # (the block before a pair block is never one that carries)
            between = np.arange(spikes[0] + 1, spikes[-1])
            free = int(np.count_nonzero(~blank[b][between])) if len(between) else 0
            d = spikes[-1] - spikes[0]
            assert free == max(0, d - pre - post - 1), (label, free)
            assert free == {'pair0': 0, 'pair1': 0, 'pair2': 1}[label]
    # every triple as a call of its own (as the GPU test runs it) and in its 16-block arrangement: the
    # carries named above arrive in both
    for k in range(0, len(blocks), 3):
        _, c3, _, _ = _same_as_brute(blocks[k:k + 3], PC.GEO_THRESH_DB, pre, post, PC.GEO_MAX_FRAC)
        _, c16, _, _ = _same_as_brute(PC.spread16(blocks[k:k + 3], 4000 + k), PC.GEO_THRESH_DB, pre, post,
                                      PC.GEO_MAX_FRAC)
        for i, want in PC.carries_of(labels[k:k + 3], post):
            assert c3[i + 1] == want and c16[(0, 7, 15)[i] + 1] == want, (labels[k:k + 3], c3, c16)


@pytest.mark.parametrize('n', PC.RAW_LENGTHS)
def test_raw_input_cases(n):
    from gpsmi import synth
    spiked = synth.raw_to_c64(PC.raw_blocks(n, True))
    assert np.array_equal(spiked, ifx_ref.raw_to_c64(PC.raw_blocks(n, True)))
    for pre, post in PC.RAW_GUARDS:
        y, counts, floors, blank = _same_as_brute(spiked, 10.0, pre, post, 1.0)
        assert (counts > 0).all()
        for b, x in enumerate(PC.raw_blocks(n, True)):
            at = np.flatnonzero(x == 0xFFFF)
            assert len(at) >= 1 and blank[b][at].all()
    flat = synth.raw_to_c64(PC.raw_blocks(n, False))
    for pre, post in PC.RAW_TIE_GUARDS:
        y, counts, floors, blank = _same_as_brute(flat, 0.0, pre, post, 1.0)
        for b, x in enumerate(flat):
            p = R.power(x)
            ties = p == floors[b]
            assert ties.sum() > 1                        # ties at the rank ...
            if (pre, post) == (0, 0):                   # ... none of them a detection: > is strict
                assert not blank[b][ties].any() and np.array_equal(blank[b], p > floors[b])
                assert 0 < counts[b] < n // 2 + 1


@pytest.mark.parametrize('thresh_db', PC.SELECT_THRESH_DB)
def test_select_cases(thresh_db):
    blocks = PC.select_blocks()
    assert len(blocks) == len(PC.SELECT_LABELS)
    pre, post = PC.SELECT_GUARD
    y, counts, floors, blank = _same_as_brute(blocks, thresh_db, pre, post, 1.0)
    p = [R.power(x) for x in blocks]
    key = [q.view(np.uint32) for q in p]
    assert len(np.unique(key[0] >> 10)) <= 2            # unit: the last pass decides
    assert np.unique(p[2]).tolist() == [0.25, 1.0] and floors[2] == 0.25
    assert np.count_nonzero(p[2] == 0.25) == (PC.SELECT_N - 1) // 2 + 1
    assert np.isnan(p[3]).sum() == 3 and np.isinf(p[3]).sum() == 2 and np.isfinite(floors[3])
    tiny = np.finfo(np.float32).tiny
    assert (p[4] < tiny).all() and (p[4] > 0).sum() > PC.SELECT_N // 2 and 0 < floors[4] < tiny
    if thresh_db == 3.0:
        assert counts[1] > 0 and counts[2] > 0 and counts[4] > 0
        assert blank[3][[64, 1500]].all()                # the infinite samples are detections


def test_carry_out_of_a_block_that_passed_through():
    c = PC.CARRY
    blocks = PC.carry_blocks()
    y, counts, floors, blank = _same_as_brute(blocks, c['thresh_db'], c['pre'], c['post'], c['max_frac'])
    assert counts.tolist() == [-1, 1024]
    assert blank[1][:1024].all() and not blank[1][1024:].any()
    assert y[0].tobytes() == blocks[0].tobytes()


def test_chunking_case():
    c = PC.CHUNK
    blocks = PC.chunk_blocks()
    assert blocks.shape == (16, c['n']) and blocks[0].nbytes * 16 > (1 << 20) > blocks[0].nbytes * 2
    y, counts, floors, blank = _same_as_brute(blocks, c['thresh_db'], c['pre'], c['post'], c['max_frac'])
    assert counts[0] == 1025 and (counts[1:] == 2049).all()
