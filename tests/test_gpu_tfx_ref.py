"""The sweep-excision kernels (gpsmi_tfx_*, csrc/gpsmi_tfx.hip) held to the float64 restatement
(tests/tfx_ref.py) at every block length, frame length, input format and kind of input of its case
table, three chained blocks each.

Per block: the cell powers (gpsmi_tfx_last_power) against the reference's; the floor, mask and count
against the float32 restatement of select / threshold / widen / count on that very P (exactly); the
mask against the reference's (outside the borderline band); the output against the reference's output
under the kernel's mask.  The bounds are FACTOR times the deviation of a float32 oracle (complex64
pocketfft transforms, float32 window and powers) from float64 on the same case, worst block."""
import numpy as np
import pytest

import tfx_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4                      # as tests/test_gpu_excision_ref.py


def _config(n):
    from gpsmi.engine import Config
    cs = 16368 if n % 16368 == 0 else 1024
    return Config(code_samples=cs, n_cyc=n // cs)


def _handle(name, **kw):
    from gpsmi.tfexcision import SweepExcision
    c = R.CASES[name]
    return SweepExcision(_config(c['n']), frame=c['L'], raw_u8=c['fmt'] == 'u8', keep_power=True,
                         **dict(c['params'], **kw))


def _given(name):
    x, raw = R.case_input(name)
    return x if raw is None else raw


def _report(title, rows):
    print(f'\n{title}')
    print(f'    {"block":<6} {"field":<6} {"kernel":>10} {"bound":>10} {"ratio":>7}')
    for b, k, err, bound in rows:
        print(f'    {b:<6} {k:<6} {err:>10.3e} {bound:>10.3e} {err / bound if bound > 0 else 0.0:>7.3f}')


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_case_against_float64(name):
    c, p = R.CASES[name], R.CASES[name]['params']
    n, L = c['n'], c['L']
    x = R.case_input(name)[0]
    sx = _handle(name)
    y = sx.apply(_given(name))
    counts, floors, masks, power = sx.last_counts.copy(), sx.last_floors.copy(), sx.last_masks.copy(), sx.last_power()
    sx.close()
    assert power.dtype == np.float32 and power.shape == (R.NB, 2 * n // L, L)
    recs = R.reference(name)
    pow_worst, out_worst = R.oracle_worst(name)
    pow_bound, out_bound = FACTOR * pow_worst, FACTOR * out_worst
    rows, moved = [], 0
    for b, r in enumerate(recs):
        gm, count = R.words_to_mask(masks[b], L), int(counts[b])
        # select, threshold, widen and count on the kernel's own P, exactly
        f32, m32, c32 = R.detect_from_power(power[b], **p)
        assert floors[b].tobytes() == np.float32(f32).tobytes(), (name, b, floors[b], f32)
        assert count == c32 and np.array_equal(gm, m32), (name, b, count, c32)
        err = R.power_metric(power[b], r['P'])
        rows.append((b, 'power', err, pow_bound))
        assert err <= pow_bound, (name, b, 'power', err, pow_bound)
        # the reference's mask, but around the cells whose P is within the power bound of its threshold
        band = R.borderline(r, pow_bound)
        assert band.sum() <= R.BORDERLINE_CAP, (name, b, int(band.sum()))
        assert count >= 0 and r['count'] >= 0, (name, b, count, r['count'])
        diff = gm != r['mask']
        assert not (diff & ~R.widen(band, p['dilate'])).any(), (name, b, np.argwhere(diff)[:8], np.argwhere(band))
        moved += int(diff.any())
        # the output under the kernel's mask
        ref = R.SweepRef(n, L, **p)
        ref.carry = r['carry']
        y_ref = r['y'] if not diff.any() else ref.excise_with(x[b], gm)
        err = float(np.abs(y[b] - y_ref).max()) / R.rms(x[b])
        rows.append((b, 'out', err, out_bound))
        assert err <= out_bound, (name, b, 'out', err, out_bound)
    _report(f'{name}: counts {counts.tolist()} of {2 * n} cells; {moved} block(s) with a borderline cell moved', rows)
    if c['kind'] == 'noise':
        assert (counts <= 2 * n // 1000).all()
    elif c['kind'] == 'pulses':                                  # (block 0 of a short block may see none)
        assert (counts[1:] > 0).all()
    else:
        assert (counts > 0).all()
    if c['kind'] == 'pulses':                                    # whole frames are flagged
        assert all(R.words_to_mask(masks[b], L).all(axis=1).any() for b in (1, 2)), name


def test_last_power_needs_keep_power_and_a_call():
    from gpsmi.engine import EngineError
    from gpsmi.tfexcision import SweepExcision
    name = 'noise-1024-L32-c64'
    sx = _handle(name)
    with pytest.raises(EngineError, match=r'\(-3\)'):
        sx.last_power()
    sx.apply(_given(name)[:1])
    assert sx.last_power().shape == (1, 64, 32)
    sx.close()
    sx = SweepExcision(_config(1024), frame=32)
    sx.apply(_given(name))
    with pytest.raises(EngineError, match=r'\(-3\).*keep_power'):
        sx.last_power()
    sx.close()
