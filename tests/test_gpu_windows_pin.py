"""GPU: the three stages on refined records -- cancellation, signatures, profiles (DESIGN.md 4.2j,
4.2p, 4.2r) -- held bit for bit to tests/golden/windows_pin.npz, which tools/record_windows_pin.py
wrote on an MI355X with the library from before the stages' host side was folded into
csrc/gpsmi_windows.h.  Nothing of the device code changed with that, so there is no tolerance:
every array is compared with array_equal.

Inputs: seeded noise (complex64, and the recorder's uint16), a row length of its own per stage, about
12 code periods at 2048 and 6 at 16368; both input formats, the host and the `_dev` entry points (which
gave the same bytes when the fixture was recorded: it holds one set for both).
  cancel     two satellites, one with a negative tau, f_offset != 0, with the coefficients.
  signature  A = 3; three records, PRN 4 twice, one tau beyond a code period, one on a half-sample
             tie; n_ms 0 and 3; cov, n_win and the prompts.
  profile    half_taps 8 and 12 (the second takes the 32-tap build), coh_ms 3, skip_ms 0 and 2, n_runs 0
             and 1; cov, n_runs and the sums.  Between two equal signature calls on the same handle a
             profile call runs on the buffers they share: the signatures stay what they were.
An array of more than 4 KiB -- the cancelled samples, the profiles' covariances -- is held by its SHA-256
(`<name>_sha256`), so that the fixture stays small."""
import hashlib

import numpy as np
import pytest

from test_gpu_acq_noncoherent import CFG, _upload

pytestmark = pytest.mark.gpu

SEED = 20250914
PERIODS = {2048: 12, 16368: 6}
EXTRA = {'cancel': 77, 'sig': 123, 'prof': 41}          # samples behind the whole periods
F_OFFSET = 1500.0
CANCEL_SATS = [(7, 2250.0, -700.3), (21, -3125.5, 611.75)]
PROF_SATS = [(4, 0, 1000.0, -300.5), (9, 2, -2750.0, 40.25), (4, 2, 3000.0, 1234.0)]
COMBOS = [(cs, raw, dev) for cs in (2048, 16368) for raw in (False, True) for dev in (False, True)]


def sig_sats(cs):
    return [(4, 1000.0, 10.5), (9, -2750.0, cs + 300.25), (4, 3000.0, -5.75)]


def rows_of(cs, stage, raw, rows=1):
    """The stage's input, [rows][n] (one row: [n]), in the input format."""
    n = PERIODS[cs] * cs + EXTRA[stage]
    rng = np.random.default_rng([SEED, cs, EXTRA[stage], int(raw)])
    if raw:
        x = rng.integers(0, 1 << 16, size=(rows, n), dtype=np.uint16)
    else:
        x = (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))).astype(np.complex64)
    return x[0] if rows == 1 else x


def run_combo(e, cs, raw, dev):
    """Every pinned call of one (code length, input format, entry point) -> {name: array}."""
    from gpsmi.engine import DeviceBuffer
    out, held = {}, []

    def arg(x):                                     # the data as the entry point takes it
        if not dev:
            return x
        held.append(_upload(x))
        return held[-1].ptr, x.shape[-1]

    try:
        x = rows_of(cs, 'cancel', raw)
        if dev:
            d_y = DeviceBuffer(x.size * 8)
            held.append(d_y)
            _, rec, coef = e.cancel(arg(x), CANCEL_SATS, out=d_y.ptr, f_offset=F_OFFSET, coef=True)
            y = d_y.download(np.complex64, x.size)
        else:
            y, rec, coef = e.cancel(x, CANCEL_SATS, f_offset=F_OFFSET, coef=True)
        out['cancel_y'], out['cancel_rec'], out['cancel_coef'] = y, rec, coef
        xs, xp = rows_of(cs, 'sig', raw, rows=3), rows_of(cs, 'prof', raw)
        d_s, d_p = arg(xs), arg(xp)
        for n_ms in (0, 3):
            res = e.signatures(d_s, sig_sats(cs), 3, n_ms=n_ms, f_offset=F_OFFSET, prompts=True)
            out.update(zip((f'sig{n_ms}_cov', f'sig{n_ms}_n_win', f'sig{n_ms}_prompts'), res))
        for half in (8, 12):
            for n_runs in (0, 1):
                res = e.profiles(d_p, PROF_SATS, half_taps=half, coh_ms=3, n_runs=n_runs, f_offset=F_OFFSET, sums=True)
                key = f'prof{half}_{n_runs}'
                out.update(zip((key + '_cov', key + '_n_runs', key + '_sums'), res))
        again = e.signatures(d_s, sig_sats(cs), 3, n_ms=3, f_offset=F_OFFSET, prompts=True)
        out.update(zip(('sig3_again_cov', 'sig3_again_n_win', 'sig3_again_prompts'), again))
    finally:
        for b in held:
            b.free()
    return dict(pinned(k, v) for k, v in out.items())


def pinned(name, a):
    """An array as the fixture holds it: itself, or its SHA-256 where it has more than 4 KiB."""
    if a.nbytes <= 4096:
        return name, a
    return name + '_sha256', np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def tag(cs, raw):                                   # (the entry points share what the fixture holds)
    return f"{cs}_{'u8' if raw else 'c64'}"


@pytest.fixture(scope='module')
def engines():
    from gpsmi.engine import AcqEngine, Config
    made = {}

    def get(cs, raw):
        if (cs, raw) not in made:
            made[cs, raw] = AcqEngine(Config(**CFG[cs]), prns=sorted({s[0] for s in CANCEL_SATS + PROF_SATS}))
            made[cs, raw].set_input_format(raw)
        return made[cs, raw]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope='module')
def pin():
    import conftest
    return conftest.load_golden('windows_pin.npz')


@pytest.mark.parametrize('cs,raw,dev', COMBOS)
def test_stages_are_the_bytes_they_were(engines, pin, cs, raw, dev):
    got = run_combo(engines(cs, raw), cs, raw, dev)
    want = {k[len(tag(cs, raw)) + 1:]: pin[k] for k in pin.files if k.startswith(tag(cs, raw) + '_')}
    assert sorted(got) == sorted(want) and len(want) == 24
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    # the windows the cases are about: a partial first window, both n_ms, one and several runs
    assert got['cancel_rec']['n_windows'].min() >= PERIODS[cs] and got['sig3_n_win'].tolist() == [3, 3, 3]
    assert got['sig0_n_win'].min() >= PERIODS[cs] - 2 and got['sig0_n_win'].max() > 3
    assert got['prof8_1_n_runs'].tolist() == [1, 1, 1] and got['prof12_0_n_runs'].max() == (3 if cs == 2048 else 1)
    # a profile call in between, on the buffers the two stages share, leaves the signatures alone
    for k in ('cov', 'n_win', 'prompts'):
        assert np.array_equal(got['sig3_again_' + k], got['sig3_' + k]), k
