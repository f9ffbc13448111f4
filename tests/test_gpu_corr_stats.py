"""corr_stats8 (csrc/gpsmi_stats.h) on magnitudes of the test's choosing, through the diagnostic
entry gpsmi_dev_corr_stats: one 256-thread workgroup per set of 2048 magnitudes, run exactly as
the correlation kernels run it (lag t + 256 q in register q of thread t, wave = t // 64).

Every value is a small non-negative integer, every set's sum a multiple of 2048 below 2^24 and
every sum of squared deviations an integer below 2^24: mean, deviations and the argument of the
square root are then exact in float32 whatever the order of the additions, the square root is
correctly rounded on both sides, and the comparison is equality, not a tolerance.  The cases are
the ways a first-index argmax can go wrong when value and index are reduced separately: ties inside
a thread, a wave and across waves, the smaller lag held by the later wave or the later lane, the
circular neighbours at the seams of thread, register row and array, and a unique maximum in every
(wave, register row) cell."""
import ctypes as C

import numpy as np
import pytest

N = 2048
PEAK = 30                      # the planted maxima; the background is 0 .. 9 (10 after the top-up)
STATS_DTYPE = np.dtype([('argmax', np.int32), ('peak', np.float32), ('mean', np.float32),
                        ('std', np.float32), ('lo', np.float32), ('hi', np.float32)])


def _cases():
    """[(name, lags that hold the maximum, expected first lag)]"""
    c = [('all equal', None, 0)]
    for a, b in ((77, 77 + 256), (77, 77 + 1792),              # twice in one thread
                 (300, 301), (640, 640 + 63),                  # twice in one wave
                 (5, 5 + 64), (5, 5 + 192),                    # in two waves
                 (200, 300),       # the smaller lag in wave 3 (row 0), the larger in wave 0 (row 1)
                 (70, 261),        # the smaller lag in wave 1 (row 0), the larger in wave 0 (row 1)
                 (266, 515),       # one wave: the smaller lag in the later lane (10, row 1; lane 3, row 2)
                 (256 + 63, 512),  # one wave: the smaller lag in the last lane, the larger in lane 0
                 (1023, 1024), (255, 256), (0, 2047)):
        c.append((f'tie {a} {b}', (a, b), a))
    c.append(('tie in every wave', (130, 130 + 64, 130 + 128, 130 - 64), 66))
    c.append(('tie in every row', tuple(191 + 256 * q for q in range(8)), 191))
    for lag in (0, 1, 255, 256, 2047, 63, 64, 1792, 2046,      # the circular neighbours
                511, 767, 1000, 1279, 1280, 1535, 1983):
        c.append((f'peak {lag}', (lag,), lag))
    for w in range(4):                                         # every (wave, row) cell
        for q in range(8):
            lag = 64 * w + 256 * q + (7 * w + 11 * q + 3) % 64
            c.append((f'cell wave {w} row {q}', (lag,), lag))
    return c


def _sets():
    rng = np.random.default_rng(8128)
    cases = _cases()
    mags = np.empty((len(cases), N), dtype=np.float32)
    for s, (name, lags, _) in enumerate(cases):
        if lags is None:
            mags[s] = 5.0
            continue
        x = rng.integers(0, 10, N)
        x[list(lags)] = PEAK
        free = np.setdiff1d(np.arange(N), lags)
        x[rng.choice(free, (-int(x.sum())) % N, replace=False)] += 1     # the mean becomes an integer
        assert x.sum() % N == 0 and x.max() == PEAK and (x == PEAK).sum() == len(lags), name
        mags[s] = x
    return cases, mags


def _reference(mags):
    ref = np.zeros(len(mags), STATS_DTYPE)
    for s, x in enumerate(mags):
        x64 = x.astype(np.float64)
        assert x64.sum() < 2 ** 24 and x64.sum() % N == 0
        mean = x64.sum() / N
        d2 = ((x64 - mean) ** 2).sum()
        assert d2 == int(d2) and d2 < 2 ** 24
        i = int(np.argmax(x))                                   # numpy: the first index
        ref[s] = (i, x[i], mean, np.sqrt(np.float32(d2 / N)), x[(i - 1) % N], x[(i + 1) % N])
    return ref


def test_cases_are_what_they_claim():
    cases, mags = _sets()
    assert len(cases) == 64
    ref = _reference(mags)
    for (name, lags, first), r in zip(cases, ref):
        assert r['argmax'] == first, name
    cells = {(int(r['argmax']) % 256 // 64, int(r['argmax']) // 256)
             for (n, _, _), r in zip(cases, ref) if n.startswith('cell')}
    assert len(cells) == 32


@pytest.mark.gpu
def test_corr_stats8_exact_on_integer_magnitudes():
    from gpsmi import _lib
    from gpsmi.engine import DeviceBuffer
    cases, mags = _sets()
    ref = _reference(mags)
    lib = _lib.load()
    d_in, d_out = DeviceBuffer(mags.nbytes), DeviceBuffer(len(mags) * STATS_DTYPE.itemsize)
    try:
        d_in.upload(mags)
        d_out.upload(np.full(len(mags) * STATS_DTYPE.itemsize, 0xFF, dtype=np.uint8))
        _lib.check(lib.gpsmi_dev_corr_stats(0, d_in.ptr, C.c_int(len(mags)), d_out.ptr),
                   'gpsmi_dev_corr_stats')
        got = d_out.download(STATS_DTYPE, len(mags))
    finally:
        d_in.free()
        d_out.free()
    bad = [(name, k, got[s][k], ref[s][k]) for s, (name, _, _) in enumerate(cases)
           for k in STATS_DTYPE.names if got[s][k] != ref[s][k]]
    assert not bad, bad[:12]
    assert got.tobytes() == ref.tobytes()
