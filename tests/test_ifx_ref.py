"""The excision reference on its own (tests/ifx_ref.py, no GPU): the float64 restatement, the
float32 restatement of the mask pass, the float32 oracle that sets the GPU tests' bounds, and the
case table of tests/test_gpu_excision_ref.py: every case gives the outcome it claims."""
import numpy as np
import pytest

import ifx_ref as R

FACTOR = 4                      # tests/test_gpu_excision_ref.py: kernel bound = FACTOR x oracle
BORDERLINE_CAP = 2


def _names():
    R.maxbins_pair()
    return sorted(R.CASES)


def _chained(ref, xs):
    return [ref.process(x) for x in xs]


@pytest.mark.parametrize('n', [4096, 5120, 9216, 16384])
def test_empty_mask_is_the_identity_chained_blocks_included(n):
    x = R._chain(1, n, 3, 35.0, [R.TONE_BIN])
    ref = R.ExcisionRef(n, thresh_db=np.inf)
    none = np.zeros(R.L, dtype=bool)
    for b in range(3):
        assert np.abs(ref.excise_with(x[b], none) - x[b]).max() <= 1e-12 * R.rms(x[b])
        y, count, mask, _, _ = ref.process(x[b])
        assert count == 0 and not mask.any()
        assert np.abs(y - x[b]).max() <= 1e-12 * R.rms(x[b])


def test_one_call_of_k_blocks_equals_k_chained_calls():
    """The reference has no batched form: a block's output is a function of the block and of the 1024
    samples before it alone, so restarting it on any block with that carry gives the same bits."""
    n = 5120
    x = R._chain(2, n, 4, 35.0, [R.TONE_BIN])
    whole = _chained(R.ExcisionRef(n), x)
    for first in range(1, 4):
        ref = R.ExcisionRef(n)
        ref.carry = x[first - 1, -R.H:].copy()
        for b, got in enumerate(_chained(ref, x[first:]), first):
            assert got[1] == whole[b][1] and np.array_equal(got[2], whole[b][2])
            assert np.array_equal(got[0], whole[b][0])


def test_mask_words_round_trip():
    rng = np.random.default_rng(5)
    for mask in (rng.random(R.L) < 0.3, np.zeros(R.L, dtype=bool), np.ones(R.L, dtype=bool),
                 np.arange(R.L) % 32 == 31, np.arange(R.L) == 2047):
        w = R.mask_words(mask)
        assert w.dtype == np.uint32 and w.shape == (64,)
        assert np.array_equal(R.words_to_mask(w), mask)
        for k in np.flatnonzero(mask)[:5]:
            assert (int(w[k // 32]) >> (k % 32)) & 1


def test_detect_from_psd_rules():
    P = np.ones(R.L, dtype=np.float32)
    P[0] = P[2047] = P[1000] = 100.0
    mask, count, thr = R.detect_from_psd(P, 6.0, 2, 256)
    assert thr == np.float32(10.0 ** 0.6) and count == 11
    assert sorted(np.flatnonzero(mask)) == [0, 1, 2, 998, 999, 1000, 1001, 1002, 2045, 2046, 2047]
    assert R.detect_from_psd(P, 6.0, 2, 11)[1] == 11
    wide = R.detect_from_psd(P, 6.0, 2, 10)
    assert wide[1] == -1 and not wide[0].any()
    P[0] = thr                                       # strict >
    assert R.detect_from_psd(P, 6.0, 0, 256)[1] == 2
    # the median is the mean of the two middle values of the sort
    P = np.concatenate([np.full(1024, 1.0), np.full(1024, 3.0)]).astype(np.float32)
    assert R.detect_from_psd(P, 0.0, 0, 2048)[2] == np.float32(2.0)
    assert R.detect_from_psd(P, 0.0, 0, 2048)[1] == 1024
    assert R.detect_from_psd(P, -np.inf, 0, 2048)[1] == 2048
    assert R.detect_from_psd(P, np.inf, 0, 2048)[1] == 0
    zero = np.zeros(R.L, dtype=np.float32)
    assert R.detect_from_psd(zero, 6.0, 2, 256)[1] == 0 and R.detect_from_psd(zero, np.inf, 2, 0)[1] == 0


@pytest.mark.parametrize('name', _names())
def test_case_gives_the_outcome_it_claims(name):
    """Outcome classes, the float32 oracle's deviations (positive, finite: the GPU bounds are FACTOR
    times them), borderline bins at most 2 per block, and detect_from_psd on the reference's own P in
    float32 agreeing with detect outside the borderline band."""
    c = R.CASES[name]
    recs = R.reference(name)
    assert len(recs) == c['held'] == (c['nb'] if name not in R.RUNS else 14)
    if c['classes'] is not None:
        assert ''.join(R.class_of(r['count']) for r in recs) == c['classes'], [r['count'] for r in recs]
    psd_worst, out_worst = R.oracle_worst(name)
    assert np.isfinite(psd_worst) and psd_worst > 0
    if any(r['count'] > 0 and r['count'] < R.L for r in recs):
        assert np.isfinite(out_worst) and out_worst > 0
    # (float32 of P is within 2^-24 P of it, far inside the band of FACTOR x the oracle's deviation)
    assert psd_worst > 2.0 ** -24
    p = c['params']
    for b, r in enumerate(recs):
        band = R.borderline(r, FACTOR * psd_worst)
        assert band.sum() <= BORDERLINE_CAP, (name, b, int(band.sum()))
        raw = r['P'].astype(np.float32) > R.detect_from_psd(r['P'].astype(np.float32), p['thresh_db'], 0, R.L)[2]
        assert np.array_equal(raw[~band], (r['P'] > r['thr'])[~band]), (name, b)
        if not band.any():
            mask, count, _ = R.detect_from_psd(r['P'].astype(np.float32), **p)
            assert count == r['count'] and np.array_equal(mask, r['mask']), (name, b)


def test_first_short_block_after_a_reset_passes_through_jammed():
    """The contract as written: behind a zero carry a 35 dB tone starts with a step at sample 0,
    which leaks across frame 0; with 3 or 4 frames in P the block is classed wideband."""
    got = {n: R.reference(f'shape-{n}-c64')[0]['count'] for n in R.SHAPES}
    assert got[4096] == -1 and got[5120] == -1
    assert all(0 < got[n] <= 256 for n in R.SHAPES[2:])
    assert got[65536] < got[32768] < got[16384]
    for n in (4096, 5120):
        r = R.reference(f'shape-{n}-c64')[0]
        assert np.array_equal(r['y'], R.case_input(f'shape-{n}-c64')[0][0].astype(np.complex128))


def test_max_bins_boundary_pair():
    c, at, below = R.maxbins_pair()
    assert 0 < c < 256
    assert R.reference(at)[1]['count'] == c
    r = R.reference(below)[1]
    assert r['count'] == -1 and not r['mask'].any()
    assert np.array_equal(r['y'], R.case_input(below)[0][1].astype(np.complex128))


def test_widening_wraps_at_both_ends():
    """A 10 dB tone on bin 0 / 2047 fills the bin and its two neighbours (Hann); the mask is that
    widened by dilate, around the ends of the spectrum."""
    for name in ('bin0', 'bin2047', 'bin1', 'bin2046'):
        k = R.EDGE_BINS[name][0]
        for d in R.EDGE_DILATES[name]:
            r = R.reference(f'edge-{name}-d{d}')[1]
            want = np.zeros(R.L, dtype=bool)
            want[np.arange(k - 1 - d, k + 2 + d) % R.L] = True
            assert np.array_equal(r['mask'], want), (name, d)
            assert r['mask'][0] and r['mask'][2047] and r['count'] == 3 + 2 * d
            # on bins 1 and 2046 a widening that clamped at the ends would give another mask
            raw = r['P'] > r['thr']
            clamped = np.array([raw[np.clip(np.arange(j - d, j + d + 1), 0, R.L - 1)].any() for j in range(R.L)])
            assert np.array_equal(clamped, want) == (name in ('bin0', 'bin2047')), (name, d)
    for name, bins in R.EDGE_BINS.items():
        if 2 not in R.EDGE_DILATES.get(name, (2,)):
            continue
        r = R.reference(f'edge-{name}-d2')[1]
        want = np.zeros(R.L, dtype=bool)
        for k in bins:
            want[np.arange(k - 3, k + 4) % R.L] = True
        assert np.array_equal(r['mask'], want), name


def test_median_is_the_mean_of_the_two_middle_values():
    """thresh_db 0, no widening: 1024 bins lie above the mean of the two middle values, 1023 above
    the upper one alone."""
    for r in R.reference('param-t0-d0-m2048'):
        assert r['count'] == R.L // 2
        assert R.detect_from_psd(r['P'].astype(np.float32), 0.0, 0, R.L)[1] == R.L // 2


def test_run_length_table():
    """The tiled cases reach the run lengths they are named for, and their chained form stays at 1."""
    want = {'run-S2': (4100, 2), 'run-S4': (8195, 4), 'run-S8': (16400, 8), 'run-S8-clipped': (16384, 8),
            'run-S1-under': (4092, 1)}
    for name, (n, nb, _) in R.RUNS.items():
        nf = n // R.H
        assert (nb * nf, R.run_length(n, nb)) == want[name] and R.RUN_S[name] == want[name][1]
        assert R.run_length(n, 4095 // nf) == 1
    assert R.RUNS['run-S8-clipped'][0] // R.H < 8             # S > nf
    x = R.case_input('run-S2')[0]
    assert np.array_equal(x[:7], x[7:14]) and len({x[b].tobytes() for b in range(7)}) == 7
