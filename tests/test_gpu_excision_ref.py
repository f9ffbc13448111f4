"""The excision kernels (gpsmi_ifx_*, csrc/gpsmi_ifx.hip) held to the float64 restatement
(tests/ifx_ref.py) at every block length, run length, parameter and edge of its case table.

Per block: the P that the mask pass thresholded (gpsmi_ifx_last_psd) against the reference's, the
mask and count against the float32 restatement of the mask pass on that very P (exactly) and against
the reference's mask (outside the borderline band), and the output against the reference's output
under the kernel's mask.  The bounds are FACTOR times the deviation of a float32 oracle (complex64
pocketfft transforms, the kernel's sum orders) from float64 on the same case, worst block."""
import itertools

import numpy as np
import pytest

import ifx_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4                      # as tests/test_gpu_acq_ref.py
BORDERLINE_CAP = 2


def _handle(name):
    from gpsmi.engine import Config
    from gpsmi.excision import Excision
    c = R.CASES[name]
    return Excision(Config(code_samples=1024, n_cyc=c['n'] // 1024), raw_u8=c['fmt'] == 'u8', **c['params'])


def _given(name):
    """What the handle of a case is given: raw uint16 for u8, else complex64."""
    x, raw = R.case_input(name)
    return x if raw is None else raw


def _run(name):
    """One call of all the blocks behind a reset -> (y [nb, n], counts, masks, psd)."""
    ex = _handle(name)
    y = ex.apply(_given(name))
    got = (y, ex.last_counts.copy(), ex.last_masks.copy(), ex.last_psd())
    ex.close()
    return got


def _report(title, rows):
    print(f'\n{title}')
    print(f'    {"block":<6} {"field":<6} {"kernel":>10} {"bound":>10} {"ratio":>7}')
    for b, k, err, bound in rows:
        ratio = err / bound if bound > 0 else 0.0
        print(f'    {b:<6} {k:<6} {err:>10.3e} {bound:>10.3e} {ratio:>7.3f}')


def _hold(name, y, counts, masks, psd):
    """The held blocks of a case against float64; -> the number of borderline bins that differed."""
    c, p = R.CASES[name], R.CASES[name]['params']
    x = R.case_input(name)[0]
    recs = R.reference(name)
    psd_worst, out_worst = R.oracle_worst(name)
    psd_bound = FACTOR * psd_worst
    rows, flipped = [], 0
    for b, r in enumerate(recs):
        gm, count = R.words_to_mask(masks[b]), int(counts[b])
        assert psd[b].dtype == np.float32
        # the mask pass on its own P, exactly
        m32, c32, _ = R.detect_from_psd(psd[b], **p)
        assert count == c32 and np.array_equal(gm, m32), (name, b, count, c32)
        if c['classes'] is not None:
            assert R.class_of(count) == c['classes'][b], (name, b, count)
        if r['psd_dev'] is None:                         # an all-zero block
            assert not psd[b].any() and count == 0 and not y[b].any(), (name, b)
            continue
        err = R.psd_metric(psd[b], r['P'])
        rows.append((b, 'psd', err, psd_bound))
        assert err <= psd_bound, (name, b, 'psd', err, psd_bound)
        # the reference's mask, but for the bins whose P is within the PSD bound of its threshold
        band = np.flatnonzero(R.borderline(r, psd_bound))
        assert len(band) <= BORDERLINE_CAP, (name, b, band)
        raw = r['P'] > r['thr']
        allowed = []
        for flips in itertools.product((False, True), repeat=len(band)):
            alt = raw.copy()
            alt[band] ^= np.array(flips, dtype=bool)
            allowed.append(R.widen_and_count(alt, p['dilate'], p['max_bins']))
        assert any(count == ac and np.array_equal(gm, am) for am, ac in allowed), \
            (name, b, count, r['count'], np.flatnonzero(gm != r['mask']), band)
        same = count == r['count'] and np.array_equal(gm, r['mask'])
        flipped += 0 if same else 1
        # the output under the kernel's mask
        if count < 0:
            assert y[b].tobytes() == x[b].tobytes(), (name, b, 'a wideband block passes through')
            continue
        if same:
            y_ref = r['y']
        else:
            ref = R.ExcisionRef(c['n'], **p)
            ref.carry = r['carry']
            y_ref = ref.excise_with(x[b], gm)
        err = float(np.abs(y[b] - y_ref).max()) / R.rms(x[b])
        bound = FACTOR * out_worst
        rows.append((b, 'out', err, bound))
        assert err <= bound, (name, b, 'out', err, bound)
        if count == R.L:
            assert not y[b].any(), (name, b, 'every bin removed')
    _report(f'{name}: n {c["n"]}, {c["fmt"]}, {p}; {flipped} block(s) with a borderline bin on the other side', rows)
    return flipped


def test_last_psd_before_the_first_call():
    from gpsmi.engine import EngineError
    ex = _handle('shape-4096-c64')
    with pytest.raises(EngineError, match=r'\(-3\)'):
        ex.last_psd()
    ex.apply(_given('shape-4096-c64')[:1])
    assert ex.last_psd().shape == (1, R.L)
    ex.apply(_given('shape-4096-c64'))
    assert ex.last_psd().shape == (3, R.L)
    ex.close()


# (a) block lengths, both formats: three chained blocks in one call behind a reset
@pytest.mark.parametrize('fmt', ['c64', 'u8'])
@pytest.mark.parametrize('n', R.SHAPES)
def test_shape_matrix(n, fmt):
    name = f'shape-{n}-{fmt}'
    _hold(name, *_run(name))


# (b) run lengths: one call of nb blocks against chained calls at S = 1, bytewise
@pytest.mark.parametrize('name', sorted(R.RUNS))
def test_run_length_does_not_change_a_bit(name):
    from gpsmi.engine import DeviceBuffer
    c = R.CASES[name]
    n, nb, nf = c['n'], c['nb'], c['n'] // R.H
    assert R.run_length(n, nb) == R.RUN_S[name]
    given = R.tile_to(_given(name), nb)
    isz = given.dtype.itemsize
    d_in, d_out = DeviceBuffer(given.nbytes), DeviceBuffer(nb * n * 8)
    try:
        d_in.upload(given)
        del given
        ex = _handle(name)
        ex.apply_dev(d_in.ptr, d_out.ptr, nb)
        whole = d_out.download(np.complex64, nb * n)
        counts, masks, psd = ex.last_counts.copy(), ex.last_masks.copy(), ex.last_psd()
        ex.reset()
        step = 4095 // nf
        assert R.run_length(n, step) == 1
        ccounts, cmasks, cpsd = [], [], []
        for b0 in range(0, nb, step):
            k = min(step, nb - b0)
            ex.apply_dev(d_in.at(b0 * n * isz), d_out.at(b0 * n * 8), k)
            ccounts.append(ex.last_counts.copy())
            cmasks.append(ex.last_masks.copy())
            cpsd.append(ex.last_psd())
        chained = d_out.download(np.complex64, nb * n)
        ex.close()
    finally:
        d_in.free()
        d_out.free()
    assert np.array_equal(counts, np.concatenate(ccounts))
    assert masks.tobytes() == np.concatenate(cmasks).tobytes()
    assert psd.tobytes() == np.concatenate(cpsd).tobytes()
    diff = np.flatnonzero(whole.view(np.uint64) != chained.view(np.uint64))
    assert not len(diff), (name, 'first differing sample', int(diff[0]), 'block', int(diff[0]) // n,
                           'segment', int(diff[0]) % n // R.H, len(diff))
    # every period repeats the second one (the first stands behind the reset)
    per = np.arange(7, nb - nb % 7).reshape(-1, 7)
    assert (counts[per] == counts[7:14]).all() and (counts > 0).sum() >= 4 * (nb // 7)
    held = c['held']
    _hold(name, whole[:held * n].reshape(held, n), counts, masks, psd)


# (c) parameters and bin edges
def _param_names():
    return sorted(k for k in R.CASES if k.startswith(('edge-bin', 'param-')) and 'maxbins' not in k)


@pytest.mark.parametrize('name', _param_names())
def test_parameters_and_bin_edges(name):
    y, counts, masks, psd = _run(name)
    _hold(name, y, counts, masks, psd)
    p = R.CASES[name]['params']
    gm = R.words_to_mask(masks[1])
    if name.split('-')[1] in R.EDGE_DILATES and 'bins' not in name:     # the wrap, at both ends
        k, d = R.EDGE_BINS[name.split('-')[1]][0], p['dilate']
        want = np.zeros(R.L, dtype=bool)
        want[np.arange(k - 1 - d, k + 2 + d) % R.L] = True
        assert np.array_equal(gm, want) and gm[0] and gm[2047] and counts[1] == 3 + 2 * d
    if p['thresh_db'] == -np.inf:
        assert (counts == R.L).all() and (masks == 0xFFFFFFFF).all() and not y.any()
    if name == 'param-t0-d0-m2048':                  # above the mean of the two middle values
        assert (counts == R.L // 2).all()
    if p['max_bins'] == 0 and name != 'param-noise-m0':
        assert (counts == -1).all() and not masks.any()


def test_max_bins_boundary():
    c, at, below = R.maxbins_pair()
    y, counts, masks, psd = _run(at)
    _hold(at, y, counts, masks, psd)
    assert counts[1] == c
    y, counts, masks, psd = _run(below)
    _hold(below, y, counts, masks, psd)
    assert counts[1] == -1 and not masks[1].any()
    assert y[1].tobytes() == R.case_input(below)[0][1].tobytes()


# (d) edges
@pytest.mark.parametrize('name', ['edge-zero-then-jammed', 'edge-wideband-middle-c64', 'edge-wideband-middle-u8'])
def test_zero_and_wideband_blocks_inside_a_call(name):
    y, counts, masks, psd = _run(name)
    _hold(name, y, counts, masks, psd)
    x = R.case_input(name)[0]
    if 'wideband' in name:
        # the block passes through as the bytes of its decode; its successor's carry is its input
        assert counts[1] == -1 and y[1].tobytes() == x[1].tobytes()
        r = R.reference(name)[2]
        assert counts[2] > 0 and np.array_equal(r['carry'], x[1, -R.H:].astype(np.complex128))
    else:
        assert counts[0] == 0 and not y[0].any() and counts[1] > 0


def test_format_switch_keeps_the_carry():
    name = 'edge-format-switch'
    x = R.case_input(name)[0]
    raw = R.quantise(x.astype(np.complex128))
    assert R.raw_to_c64(raw).tobytes() == x.tobytes()
    y, counts, masks, psd = _run(name)
    _hold(name, y, counts, masks, psd)
    from gpsmi._lib import check
    for first_u8 in (False, True):
        ex = _handle(name)
        got = []
        for b, u8 in enumerate((first_u8, not first_u8)):
            check(ex.lib.gpsmi_ifx_set_input_format(ex.h, int(u8)), 'gpsmi_ifx_set_input_format')
            ex.raw_u8 = u8
            got.append(ex.apply(raw[b] if u8 else x[b]))
            assert ex.last_counts[0] == counts[b] and np.array_equal(ex.last_masks[0], masks[b])
            assert ex.last_psd().tobytes() == psd[b].tobytes()
        ex.close()
        assert np.stack(got).tobytes() == y.tobytes()


def test_calls_of_one_and_three_blocks_equal_one_of_four():
    name = 'edge-1-plus-3'
    y, counts, masks, psd = _run(name)
    _hold(name, y, counts, masks, psd)
    x = _given(name)
    ex = _handle(name)
    y0 = ex.apply(x[:1])
    c0, m0, p0 = ex.last_counts.copy(), ex.last_masks.copy(), ex.last_psd()
    y1 = ex.apply(x[1:])
    assert np.concatenate([y0, y1]).tobytes() == y.tobytes()
    assert np.array_equal(np.concatenate([c0, ex.last_counts]), counts)
    assert np.concatenate([m0, ex.last_masks]).tobytes() == masks.tobytes()
    assert np.concatenate([p0, ex.last_psd()]).tobytes() == psd.tobytes()
    ex.close()
