"""GPU: the multi-antenna stage -- one weight per antenna, space-time taps, per-satellite beams
 -- held bit for bit to tests/golden/nul_pin.npz, which
tools/record_nul_pin.py wrote on an MI355X with the library from before the three forms were given one
solve core and one call skeleton.  The kernels have no atomics and the order of their sums is fixed by
the block length alone, so there is no tolerance: every array is compared with array_equal.

Inputs: the blocks of test_gpu_nulling.py's matrix and the beams of test_gpu_beams.py's, seeded.  Two
block lengths, three blocks a call, one of which at least passes through (flags 0 and 1 both occur):
  2048     the shortest block: one slice of the covariance, less than one workgroup of the raw apply.
  10272    8192 + 2080: two slices, the second short; a partial last workgroup in every apply kernel;
           no multiple of the 256 samples the space-time covariance stages at a time.
Cases, each in both input formats:
  weights  A in (2, 3, 5, 8) with one weight per antenna, A in (2, 8) with 3, 5 and 7 taps; the host
           and the `_dev` entry point (which gave the same bytes when the fixture was recorded: it
           holds one set for both).  Output, flags, gain, weights.
  beams    A in (2, 3, 5, 8), 3 and 16 beams whose masks carry 0, 1 and min(A - 1, 4) nulls; the host
           entry, beams_dev on packed rows, and beams_dev on rows 64 (in) and 34 (out) samples apart,
           where what stands between the output rows must be left as it was.  One set for all three.
  flag -1  test_gpu_beams.test_a_beam_without_weights_is_zeros' case (A = 2, n = 2048).
  apply, beams, the same apply again on one handle: the second apply is the first.
An array of more than 4 KiB -- the outputs, the weights of 16 beams -- is held by its SHA-256
(`<name>_sha256`), so that the fixture stays small."""
import functools
import hashlib

import numpy as np
import pytest

import nul_ref as R
from test_gpu_beams import _beams_for
from test_gpu_nulling import JN_DB, SIGMA, _case_blocks, _cfg

pytestmark = pytest.mark.gpu

NS = (2048, 10272)
MIX = {2048: 0, 10272: 1}       # which of _case_blocks' three mixes of blocks a length takes
NB = 3
NBEAMS = (3, 16)
GAP_IN, GAP_OUT = 64, 34        # samples between the rows of the strided beams call (even)
FILL = np.complex64(7.0 - 3.0j)
KEYS = ('y', 'flags', 'gain', 'w')

WEIGHTS = [(A, 1) for A in (2, 3, 5, 8)] + [(A, T) for T in (3, 5, 7) for A in (2, 8)]
WEIGHT_CASES = [(A, T, raw, dev) for A, T in WEIGHTS for raw in (False, True) for dev in (False, True)]
BEAM_CASES = [(A, raw, entry) for A in (2, 3, 5, 8) for raw in (False, True)
              for entry in ('host', 'dev', 'strided')]


@functools.lru_cache(maxsize=None)
def blocks(A, n, raw):
    """[A][NB * n] in the input format (shared by the cases: never written to)."""
    x = _case_blocks(A, n, NB, raw, mix=MIX[n])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def beams_of(A, nbeam):
    return _beams_for(A, nbeam, 17 * A + nbeam)


def pinned(name, a):
    """An array as the fixture holds it: itself, or its SHA-256 where it has more than 4 KiB."""
    a = np.ascontiguousarray(a)
    if a.nbytes <= 4096:
        return name, a
    return name + '_sha256', np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)


def pinned_all(name, per_length):
    """One entry of the fixture for both block lengths: what pinned() makes of each, stacked."""
    made = [pinned(name, a) for a in per_length]
    return made[0][0], np.stack([a for _, a in made])


def weights_tag(A, T, raw):                         # (the entry points share what the fixture holds)
    return f"w{T}_A{A}_{'u8' if raw else 'c64'}"


def beams_tag(A, raw):
    return f"beams_A{A}_{'u8' if raw else 'c64'}"


def apply_once(ns, x, n, dev):
    """One gpsmi_nul_apply / _apply_dev call on NB blocks -> output, flags, gain, weights."""
    from gpsmi.engine import DeviceBuffer
    if not dev:
        y = ns.apply(x).ravel()
    else:
        d_in, d_out = DeviceBuffer(x.nbytes), DeviceBuffer(NB * n * 8)
        try:
            d_in.upload(x)
            ns.apply_dev(d_in.ptr, d_out.ptr, NB)
            y = d_out.download(np.complex64, NB * n)
        finally:
            d_in.free()
            d_out.free()
    return y, ns.last_flags.copy(), ns.last_gain_db.copy(), ns.last_weights.copy()


def run_weights(A, T, raw, dev):
    """Both block lengths of one (antennas, taps, input format, entry point) -> {name: array}."""
    from gpsmi.nulling import NullSteer
    res = []
    for n in NS:
        ns = NullSteer(_cfg(n), antennas=A, raw_u8=raw, taps=T)
        try:
            res.append(apply_once(ns, blocks(A, n, raw), n, dev))
        finally:
            ns.close()
    return dict(pinned_all(k, v) for k, v in zip(KEYS, zip(*res)))


def beams_once(ns, x, n, A, beams, entry):
    """One beams call on NB blocks by the host entry, beams_dev on packed rows or beams_dev on rows
    GAP_IN / GAP_OUT samples apart -> output [nbeam][NB * n], flags, gain, weights."""
    from gpsmi.engine import DeviceBuffer
    nbeam, row = len(beams[0]), NB * n
    if entry == 'host':
        y = ns.beams(x, *beams)
    else:
        gi, go = (GAP_IN, GAP_OUT) if entry == 'strided' else (0, 0)
        wide = np.zeros((A, row + gi), dtype=x.dtype)
        wide[:, :row] = x
        wide[:, row:] = x[:, :gi]                   # (what stands between the rows is no block)
        d_in, d_out = DeviceBuffer(wide.nbytes), DeviceBuffer(nbeam * (row + go) * 8)
        try:
            d_in.upload(wide)
            d_out.upload(np.full(nbeam * (row + go), FILL))
            ns.beams_dev(d_in.ptr, d_out.ptr, NB, *beams, in_stride=row + gi, out_stride=row + go)
            got = d_out.download(np.complex64, nbeam * (row + go)).reshape(nbeam, row + go)
        finally:
            d_in.free()
            d_out.free()
        assert (got[:, row:] == FILL).all(), 'the samples between the output rows were written'
        y = np.ascontiguousarray(got[:, :row])
    return y, ns.last_beam_flags.copy(), ns.last_beam_gain_db.copy(), ns.last_beam_weights.copy()


def run_beams(A, raw, entry):
    """Both block lengths and both beam counts of one (antennas, input format, entry) -> {name: array}."""
    from gpsmi.nulling import NullSteer
    res = {nbeam: [] for nbeam in NBEAMS}
    for n in NS:
        ns = NullSteer(_cfg(n), antennas=A, raw_u8=raw)
        try:
            for nbeam in NBEAMS:
                res[nbeam].append(beams_once(ns, blocks(A, n, raw), n, A, beams_of(A, nbeam), entry))
        finally:
            ns.close()
    return dict(pinned_all(f'b{nbeam}_{k}', v) for nbeam in NBEAMS for k, v in zip(KEYS, zip(*res[nbeam])))


def run_no_weights():
    """test_gpu_beams.test_a_beam_without_weights_is_zeros' call -> {name: array}."""
    from gpsmi.nulling import NullSteer
    A, n = 2, 2048
    rng = np.random.default_rng(9)
    x = (1.0e30 * R.cgauss(rng, (A, 2 * n))).astype(np.complex64)
    x[:, n:] = R.noisy_block(rng, A, n, 1, JN_DB, SIGMA)
    steer = np.stack([R.cgauss(rng, A) * 1.0e-150, R.cgauss(rng, A)])
    ns = NullSteer(_cfg(n), antennas=A)
    try:
        y = ns.beams(x, steer)
        res = (y, ns.last_beam_flags.copy(), ns.last_beam_gain_db.copy(), ns.last_beam_weights.copy())
    finally:
        ns.close()
    return dict(pinned(k, v) for k, v in zip(KEYS, res))


@pytest.fixture(scope='module')
def pin():
    import conftest
    return conftest.load_golden('nul_pin.npz')


def held(pin, tag):
    return {k[len(tag) + 1:]: pin[k] for k in pin.files if k.startswith(tag + '_')}


def same(got, want, count):
    assert sorted(got) == sorted(want) and len(want) == count
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize('A,T,raw,dev', WEIGHT_CASES,
                         ids=[f'A{A}-T{T}-{"u8" if r else "c64"}-{"dev" if d else "host"}' for A, T, r, d in WEIGHT_CASES])
def test_weights_are_the_bytes_they_were(pin, A, T, raw, dev):
    want = held(pin, weights_tag(A, T, raw))
    same(run_weights(A, T, raw, dev), want, 4)
    assert want['flags'].shape == (len(NS), NB) and set(want['flags'].ravel().tolist()) == {0, 1}      # nulled and passed through


@pytest.mark.parametrize('A,raw,entry', BEAM_CASES,
                         ids=[f'A{A}-{"u8" if r else "c64"}-{e}' for A, r, e in BEAM_CASES])
def test_beams_are_the_bytes_they_were(pin, A, raw, entry):
    same(run_beams(A, raw, entry), held(pin, beams_tag(A, raw)), 8)


def test_a_beam_without_weights_is_the_bytes_it_was(pin):
    want = held(pin, 'none')
    same(run_no_weights(), want, 4)
    assert want['flags'].tolist() == [[-1, 1], [1, 1]]
    # adaptive, quiescent and without weights: every flag of a beam occurs in the fixture
    seen = set(want['flags'].ravel().tolist())
    for A, raw, _ in BEAM_CASES:
        for nbeam in NBEAMS:
            f = held(pin, beams_tag(A, raw))[f'b{nbeam}_flags']
            assert f.shape == (len(NS), NB, nbeam)
            seen |= set(f.ravel().tolist())
    assert seen == {-1, 0, 1}


def test_a_beams_call_in_between_leaves_apply_alone(pin):
    from gpsmi.nulling import NullSteer
    A, n = 3, 10272
    x = blocks(A, n, False)
    ns = NullSteer(_cfg(n), antennas=A)
    try:
        first = apply_once(ns, x, n, False)
        ns.beams(x, *beams_of(A, 3))
        kept = (ns.last_flags.copy(), ns.last_gain_db.copy(), ns.last_weights.copy())
        again = apply_once(ns, x, n, False)
    finally:
        ns.close()
    for k, a, b in zip(KEYS, first, again):
        assert np.array_equal(a, b), k
    for k, a, b in zip(KEYS[1:], first[1:], kept):
        assert np.array_equal(a, b), k
    want = held(pin, weights_tag(A, 1, False))
    for k, v in dict(pinned(k, v) for k, v in zip(KEYS, again)).items():
        assert np.array_equal(v, want[k][NS.index(n)]), k
