"""GPU: bit-synchronous tracking of refined hits (gpsmi_acq_track) against the float64 restatement
(wtrk_ref.py) across its options and shapes, on the small synthetic scenes of small_scene.py.
test_gpu_acq_track.py pins the deep scene at the defaults over 45 bits; here every case exists for
something that scene never reaches:

    ring      60 bits > GPSMI_WTRK_RING = 50: the C/N0 ring wraps, in one call and in chunks
    options   non-default gains; the PLL, the FLL and the pull-in switched off; a wide DLL
    taps      1 and 15 samples at 16368
    slide     f_offset -+3 MHz, once with the L2 carrier: windows sliding 4 .. 31 samples per ms
    many      64 channels; data that ends so that about half of them stop after bit 2
    far       first_sample = 2^31 + 4096: the double -> long long window arithmetic past 2^31

Channels are opened by open_ref from refine_ref on the first 100 ms of the same data.  As in
test_gpu_acq_track.py every window start the GPU used is compared exactly, for every bit;
test_acq_track.py asserts on the CPU that the restatement's s_k stay clear of the integers.

Numbers.  Prompts, f_hz, tau and cn0 are held to the TOL table of test_gpu_acq_track.py as it stands
(in the far case tau plus two ulp of tau, 2 x 4.8e-7 at 2^31): on the first GPU run (MI355X) every
case stayed under it, so none has a constant of its own.  The largest deviations measured then:
                      prompts / max|P|   f_hz, Hz    tau, samples   cn0, dB
    ring              7.806e-07          2.583e-06   1.956e-08      1.261e-05   (bits 50 .. 59: 2.022e-06)
    options (four)    9.755e-08          4.244e-07   1.903e-08      4.238e-06
    taps 1 / 15       8.734e-08          2.070e-07   1.211e-08      9.104e-06
    slide 2048        2.561e-07          5.101e-07   8.789e-09      1.643e-06
    slide 16368       1.784e-07          3.359e-07   4.563e-08      1.509e-06
    many (and cut)    6.813e-08          8.480e-08   1.397e-09      6.574e-06
    far               5.779e-08          7.784e-08   0              4.479e-06
The states handed back (held to the same table: tau, f_hz, f_acc under f_hz's figure, lock under
the prompts'): tau 8.475e-08, f_hz 3.717e-07, f_acc 3.717e-07, lock 1.718e-07 at most.
(DESIGN.md 4.2g has the same figures.)  The table itself lies under the caps: prompts / max|P| 1e-4,
f_hz 1e-3 Hz, tau INTEGER_GUARD / 10."""
import numpy as np
import pytest

import small_scene as S
import wtrk_ref as W
from test_acq_track import INTEGER_GUARD
from test_gpu_acq_noncoherent import _engine, _same
from test_gpu_acq_track import TOL, _cplx
from test_gpu_acq_track import deviations as _deviations

pytestmark = pytest.mark.gpu

ULP_FAR = 2.0 ** (31 - 52)
CAP = dict(prompts=1e-4, f_hz=1e-3, tau=INTEGER_GUARD / 10)

# mu_ring holds float32 values of up to 20 (here 3 .. 17: an ulp is 2.4e-7 .. 1.9e-6); the largest
# deviation from the restatement's ring on the first GPU run (MI355X) was 1.907e-06, one or two ulp;
# asserted at four times that
MU_RING_TOL = 4 * 1.907e-06
for _t in TOL.values():
    assert all(_t[k] <= CAP[k] for k in CAP)


def tolerance(case):
    """The table as it stands; in the far case tau itself has an ulp of 4.8e-7, so any deviation at
    all shows as a whole ulp: two ulp are added there, still five times below INTEGER_GUARD."""
    t = dict(TOL[case.cs])
    if case.name == 'far':
        t['tau'] += 2 * ULP_FAR
        assert t['tau'] <= CAP['tau'] + 2 * ULP_FAR
    return t


@pytest.fixture(scope='module')
def engines():
    made = {}

    def get(cs):
        if cs not in made:
            made[cs] = _engine(cs)
        return made[cs]
    yield get
    for e in made.values():
        e.close()


def engine_kw(case):
    o = dict(case.opts)
    if 'tap' in o:
        o['tap_samples'] = o.pop('tap')
    return o


def check_decisions(rec, st, ref, rst, rnk, case):
    """bit counts, flags, every window start, and the hard bits where the restatement's are clear."""
    kw = case.scene_kw()
    assert st['bit_no'].tolist() == [s['bit_no'] for s in rst]
    assert st['flags'].tolist() == [s['flags'] for s in rst]
    assert np.array_equal(st['prn'], [s['prn'] for s in rst])
    assert np.array_equal(rec['bit_no'], ref['bit_no'])
    for h in range(len(rec)):
        nb = rst[h]['bit_no']
        for b in range(nb):
            _, _, n = W.windows(rec[h, b]['tau'], rec[h, b]['f_hz'], case.cs, **kw)
            assert np.array_equal(n, rnk[h, b]), (h, b)
        assert not rec[h, nb:].view(np.uint8).any()           # the records past the last bit are zero
        clear = np.abs(ref[h, :nb]['p_i']) > 0.1 * np.abs(_cplx(ref[h, :nb], 'p')).mean()
        assert np.array_equal(rec[h, :nb]['p_i'][clear] >= 0, ref[h, :nb]['p_i'][clear] >= 0)
    for g, s in zip(st['theta'], rst):                        # (close on the circle, as the first test)
        d = (int(g) - s['theta']) % (1 << 64)
        assert min(d, (1 << 64) - d) / 2.0 ** 64 < 1e-3


def deviations(rec, ref):
    """test_gpu_acq_track's, for records that may hold no C/N0 yet (mean mu <= 1 throughout)."""
    if np.isnan(ref['cn0_dbhz']).all():
        assert np.isnan(rec['cn0_dbhz']).all()
        ref, rec = ref.copy(), rec.copy()
        ref['cn0_dbhz'][0, 0] = rec['cn0_dbhz'][0, 0] = 0.0
    return _deviations(rec, ref)


def check_numbers(rec, st, ref, rst, case, what=''):
    """The records of every bit all channels tracked, and the states handed back: tau and f_hz of
    the next bit (what its record would hold) and the loop's integrator."""
    live = [h for h in range(len(rec)) if rst[h]['bit_no'] > 0]
    nb = min(rst[h]['bit_no'] for h in live)
    dev = deviations(rec[live, :nb], ref[live, :nb])
    sdev = {k: max(abs(float(st[k][h]) - rst[h][k]) for h in range(len(rst))) for k in ('tau', 'f_hz', 'f_acc', 'lock')}
    print('deviations %s%s: ' % (case.name, what) + '  '.join('%s %.3e' % kv for kv in dev.items())
          + '   states: ' + '  '.join('%s %.3e' % kv for kv in sdev.items()))
    tol = tolerance(case)
    for k, v in dev.items():
        assert v <= tol[k], (k, v, tol[k])
    assert sdev['tau'] <= tol['tau'] and sdev['f_hz'] <= tol['f_hz'] and sdev['f_acc'] <= tol['f_hz']
    assert sdev['lock'] <= tol['prompts']              # (a ratio of prompts, smoothed)
    return dev


def mu_ring_deviation(st, rst):
    return max(np.abs(st['mu_ring'][h].astype(np.float64) - np.asarray(rst[h]['mu_ring'])).max()
               for h in range(len(rst)))


# ---- ring ----------------------------------------------------------------------------------------------

def test_ring_wraps_in_one_call_and_in_chunks(engines):
    case = S.TRACK_CASES['ring']
    c64 = case.data()[0]
    s0 = W.states_array(case.states())
    ref, rst, rnk = case.ref()
    e = engines(2048)
    rec, st = e.track_weak(c64, s0, case.n_bits)
    check_decisions(rec, st, ref, rst, rnk, case)
    check_numbers(rec, st, ref, rst, case)
    # C/N0 of the bits the ring has wrapped for, on their own
    late = np.abs(rec[:2, W.RING:]['cn0_dbhz'] - ref[:2, W.RING:]['cn0_dbhz']).max()
    dmu = mu_ring_deviation(st, rst)
    print('cn0 of bits 50 .. 59: %.3e dB   mu_ring: %.3e' % (late, dmu))
    assert late <= tolerance(case)['cn0'] and dmu <= MU_RING_TOL
    for chunks in ((30, 30), (49, 1, 10)):
        parts, s = [], s0
        for n in chunks:
            r, s = e.track_weak(c64, s, n)
            parts.append(r)
        _same(np.concatenate(parts, axis=1), rec)
        _same(s, st)


# ---- options, taps, slide --------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [n for n in S.TRACK_CASES if n.split('-')[0] in ('options', 'taps', 'slide')])
def test_case_against_the_restatement(name, engines):
    case = S.TRACK_CASES[name]
    ref, rst, rnk = case.ref()
    rec, st = engines(case.cs).track_weak(case.data()[0], W.states_array(case.states()), case.n_bits,
                                          **engine_kw(case))
    check_decisions(rec, st, ref, rst, rnk, case)
    check_numbers(rec, st, ref, rst, case)


# ---- many ------------------------------------------------------------------------------------------------

def test_64_channels_and_data_that_ends_for_half_of_them(engines):
    from gpsmi._lib import WTRK_DATA_END
    case = S.TRACK_CASES['many']
    c64 = case.data()[0]
    s0 = W.states_array(case.states())
    assert len(s0) == 64
    e = engines(2048)
    ref, rst, rnk = case.ref()
    rec, st = e.track_weak(c64, s0, case.n_bits)
    check_decisions(rec, st, ref, rst, rnk, case)
    check_numbers(rec, st, ref, rst, case)
    cut = S.many_cut(case)
    cref, crst, cnk = case.ref(n=cut)
    crec, cst = e.track_weak(c64[:cut], s0, case.n_bits)
    stopped = [h for h in range(64) if crst[h]['bit_no'] == 2]
    print('cut %d: %d channels stop after bit 2' % (cut, len(stopped)))
    assert 16 <= len(stopped) <= 48
    check_decisions(crec, cst, cref, crst, cnk, case)
    check_numbers(crec, cst, cref, crst, case, ' (cut)')
    for h in range(64):
        assert cst['flags'][h] == (WTRK_DATA_END if h in stopped else 0)
        _same(crec[h, :2], rec[h, :2])
        if h not in stopped:
            _same(crec[h], rec[h])
            _same(cst[h:h + 1], st[h:h + 1])


# ---- far -------------------------------------------------------------------------------------------------

def test_stream_positions_past_2_to_the_31(engines):
    """The same data taken to start at sample 2^31 + 4096, every tau moved with it, against the
    restatement called the same way."""
    case = S.TRACK_CASES['far']
    c64 = case.data()[0]
    near = case.states()
    far = [dict(s, tau=s['tau'] + S.FAR) for s in near]
    ref, rst, rnk = case.ref(first_sample=S.FAR)
    assert rnk.min() > 2 ** 31
    rec, st = engines(2048).track_weak(c64, W.states_array(far), case.n_bits, first_sample=S.FAR)
    check_decisions(rec, st, ref, rst, rnk, case)
    check_numbers(rec, st, ref, rst, case)
    assert np.all(rec['tau'] > 2 ** 31) and np.all(st['tau'] > 2 ** 31)
