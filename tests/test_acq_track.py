"""Bit-synchronous tracking of refined hits (gpsmi_acq_track), the parts that need no GPU: the ABI's
declarations, struct sizes and argument errors, gpsmi_wtrk_open, and the float64 restatement
(wtrk_ref.py) against the truth of the pinned deep scene at 25.5 dB-Hz (weak) and at 35 dB-Hz
(strong), its channels opened from the restatement of refinement on the same data.

Bounds on the truth, over the last 20 of 45 bits, from the restatement's own run at the default
bandwidths (PLL 4 Hz, FLL 1 Hz, DLL 0.5 Hz, 10 pull-in bits), weak scene, per channel:
    |tau error|     worst 0.169 sample (PRNs 6, 15, 23, 29, 10: 0.077 0.080 0.169 0.055 0.114)
                    asserted 0.25: the worst plus half of it
    f_hz error rms  worst 3.40 Hz (2.14 1.80 1.58 3.40 1.38); asserted 5.0: the worst plus half of it
    cn0_dbhz        23.2 .. 24.5; asserted in refinement's [22, 26]
    transitions     0 .. 2 of 44 differ from the truth (2 0 0 2 0); asserted at most 4 of 44 per
                    channel (twice the worst, 9 %)
Phase lock does not hold at 25.5 dB-Hz (sign Re P against the true bits flips up to 3 times per
channel from bit 20 on), so hard bits are asserted on the strong scene only: equal to the truth up
to one global sign from bit pull_in_bits + 10 = 20 on, lock indicator 0.46 .. 0.82 (> 0)."""
import ctypes as C

import numpy as np
import pytest

import small_scene as S
import wtrk_ref as W
from deep_ref import L1_HZ

TAU_BOUND = 0.25            # samples  (measured worst 0.169)
F_RMS_BOUND = 5.0           # Hz       (measured worst 3.40)
CN0_BAND = (22.0, 26.0)
TRANS_CAP = 4               # of 44    (measured worst 2)
LAST = 20
# every window start of the restatement stays this far from an integer (measured: 1.5e-4 weak,
# 5.7e-5 strong, 1.65e-4 at 16368), see test_gpu_acq_track.py
INTEGER_GUARD = 1e-5


def check_truth(scene, rec, prns, strong=False):
    """The bounds above on bit records [nch, 45] of the five satellites (restatement's or the
    GPU's); every figure is printed before it is asserted."""
    from gpsmi.acquisition import weak_bits
    figs = []
    for r, prn in zip(rec, prns):
        s = W.truth_of(scene, prn)
        te = np.abs(W.tau_error(scene, prn, r['tau'])[-LAST:]).max()
        fr = float(np.sqrt(np.mean((r['f_hz'][-LAST:] - s.doppler) ** 2)))
        tb = W.true_bits(scene, prn, r['tau'])
        bits, tr = weak_bits(r)
        terr = int((tr != tb[1:] * tb[:-1]).sum())
        agree = (bits * tb)[W.DEF_PULL_IN + 10:]
        figs.append((prn, te, fr, float(r['cn0_dbhz'][-1]), terr, float(r['lock'][-1]), agree))
        print('prn %2d  tau err %.3f  f rms %.2f  cn0 %.2f  transitions wrong %d  lock %.2f  bits %s'
              % (prn, te, fr, r['cn0_dbhz'][-1], terr, r['lock'][-1],
                 ''.join('+' if a > 0 else '-' for a in agree)))
    for prn, te, fr, cn0, terr, lock, agree in figs:
        assert te <= TAU_BOUND and fr <= F_RMS_BOUND
        assert terr <= TRANS_CAP
        if strong:
            assert abs(int(agree.sum())) == len(agree)          # one global sign
            assert lock > 0
        else:
            assert CN0_BAND[0] <= cn0 <= CN0_BAND[1]


# ---- the restatement against the truth --------------------------------------------------------

def test_weak_scene_holds_code_and_frequency_lock():
    sc, states, _ = W.opened()
    rec, st, _ = W.tracked()
    assert [s['bit_no'] for s in st] == [W.N_BITS] * 6 and not any(s['flags'] for s in st)
    check_truth(sc, rec[:5], [s['prn'] for s in states[:5]])


def test_strong_scene_holds_phase_lock():
    sc, states, _ = W.opened(W.STRONG_AMP)
    rec, st, _ = W.tracked(W.STRONG_AMP)
    check_truth(sc, rec[:5], [s['prn'] for s in states[:5]], strong=True)
    assert 34.5 <= 10 * np.log10(W.STRONG_AMP ** 2 * 2.048e6 / 0.35 ** 2) <= 35.5


@pytest.mark.parametrize('amp', [None, W.STRONG_AMP])
def test_absent_prn_does_not_lock(amp):
    """The sixth channel is PRN 3, not in the scene: |lock| stays below 0.5 (a smoothed cos 2 phi
    of uniform phase has sigma 0.707 sqrt(0.05 / 1.95) = 0.11: 0.5 is 4.4 sigma) and its C/N0 is
    NaN or below every present satellite's."""
    _, states, _ = W.opened(amp)
    rec, _, _ = W.tracked(amp)
    assert states[5]['prn'] == W.ABSENT[0]
    print(rec[5]['lock'], rec[5]['cn0_dbhz'][-1], rec[:5, -1]['cn0_dbhz'])
    assert np.abs(rec[5]['lock']).max() < 0.5
    c = rec[5]['cn0_dbhz'][-1]
    assert np.isnan(c) or c < rec[:5, -1]['cn0_dbhz'].min()


@pytest.mark.parametrize('amp,cs', [(None, 2048), (W.STRONG_AMP, 2048), (None, 16368)])
def test_windows_keep_clear_of_integers(amp, cs):
    """n_k = floor(s_k) is compared exactly on the GPU: the restatement's s_k must not sit where a
    deviation of the size the GPU test tolerates in tau could move the floor."""
    rec, st, nk = W.tracked(amp, cs)
    worst = 1.0
    for h in range(len(st)):
        for b in range(st[h]['bit_no']):
            _, s, n = W.windows(rec[h, b]['tau'], rec[h, b]['f_hz'], cs)
            assert np.array_equal(n, nk[h, b])
            worst = min(worst, float(np.minimum(s - n, 1.0 - (s - n)).min()))
    print('closest s_k to an integer: %.3e' % worst)
    assert worst > INTEGER_GUARD
    if cs == 2048:                               # the windows do cross integers inside the span
        assert any(len(set((nk[h, :, 0] - nk[h, 0, 0]) - 20 * cs * np.arange(nk.shape[1]))) > 3 for h in range(4))


def test_chunks_and_order_do_not_matter_to_the_restatement():
    """20 + 25 bits with the states carried over and the second chunk passed as a slice."""
    _, states, _ = W.opened()
    rec, st, _ = W.tracked()
    x = W.scene_c64()
    a, sa, _ = W.track_ref(x, states[:2], 20, 2048)
    first = int(min(np.floor(s['tau']) for s in sa)) - 1
    b, sb, _ = W.track_ref(x[first:], sa, 25, 2048, first_sample=first)
    assert np.concatenate([a, b], axis=1).tobytes() == rec[:2].tobytes()
    assert sb == st[:2]


def test_weak_bits_helper():
    from gpsmi._lib import WTRK_BIT_DTYPE
    from gpsmi.acquisition import weak_bits
    r = np.zeros(5, WTRK_BIT_DTYPE)
    r['p_i'] = [3, -2, -1, 0.1, 4]
    r['p_q'] = [0, 0, 5, -6, 0]
    bits, tr = weak_bits(r)
    assert bits.tolist() == [1, -1, -1, 1, 1]
    assert tr.tolist() == [-1, 1, -1, 1]               # Re(P_b conj P_{b-1}): -6, 2, -30.1, 0.4


# ---- ABI ----------------------------------------------------------------------------------------

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_struct_sizes():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(10) == C.sizeof(_lib.WtrkCfg) == 64
    assert lib.gpsmi_abi_sizeof(11) == _lib.WTRK_STATE_DTYPE.itemsize == 256
    assert lib.gpsmi_abi_sizeof(12) == _lib.WTRK_BIT_DTYPE.itemsize == 64
    for dt in (_lib.WTRK_STATE_DTYPE, _lib.WTRK_BIT_DTYPE):            # no implicit padding
        assert sum(dt.fields[n][0].itemsize for n in dt.names) == dt.itemsize
    covered = sum(getattr(_lib.WtrkCfg, n).size for n, _ in _lib.WtrkCfg._fields_)
    assert covered == C.sizeof(_lib.WtrkCfg)
    for name in ('gpsmi_acq_track', 'gpsmi_acq_track_dev', 'gpsmi_acq_track_plan', 'gpsmi_wtrk_open'):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_argument_errors_need_no_gpu():
    from gpsmi import _lib
    lib = _lib.load()
    st = np.zeros(65, _lib.WTRK_STATE_DTYPE)
    st['prn'], st['tau'], st['f_hz'], st['f_acc'] = 6, 412.3, -4830.0, -4830.0
    bits = np.zeros((65, 4), _lib.WTRK_BIT_DTYPE)
    buf = np.zeros(16, np.float32)
    n = 100 * 2048

    def cfg(**kw):
        d = dict(n_bits=4, tap_samples=0, pll_bw_hz=0.0, fll_bw_hz=0.0, dll_bw_hz=0.0, carrier_hz=L1_HZ,
                 f_offset_hz=0.0, first_sample=0, pull_in_bits=0, reserved=0)
        d.update(kw)
        return _lib.WtrkCfg(**d)

    def plan(cs=2048, n=n, st=st, nhits=5, c=None, want=-1, text=None):
        c = cfg() if c is None else c
        rc = lib.gpsmi_acq_track_plan(cs, n, None if st is None else _p(st), nhits,
                                      C.byref(c) if c is not False else None)
        assert rc == want, (rc, lib.gpsmi_last_error())
        if text:
            assert text in lib.gpsmi_last_error(), lib.gpsmi_last_error()

    plan(want=0)
    plan(nhits=64, want=0)
    plan(cs=16368, n=100 * 16368, want=0)
    plan(c=cfg(pll_bw_hz=-1.0, fll_bw_hz=-1.0, pull_in_bits=-1), want=0)
    plan(n=10, want=0)                                   # a channel that fits no bit is no error
    plan(st=None, text=b'null')
    plan(c=False, text=b'null')
    for fn in (lib.gpsmi_acq_track, lib.gpsmi_acq_track_dev):
        assert fn(None, _p(buf), n, _p(st), 5, C.byref(cfg()), _p(bits)) == -1
        assert b'null' in lib.gpsmi_last_error()
    plan(nhits=0, text=b'nhits')
    plan(nhits=65, text=b'nhits')
    plan(c=cfg(n_bits=0), text=b'n_bits')
    plan(c=cfg(n_bits=-3), text=b'n_bits')
    for bad in (float('nan'), float('inf'), 0.0, -1.0):
        plan(c=cfg(carrier_hz=bad), text=b'carrier_hz')
    plan(c=cfg(f_offset_hz=float('nan')), text=b'f_offset_hz')
    plan(c=cfg(dll_bw_hz=-1.0), text=b'dll_bw_hz')
    plan(c=cfg(pll_bw_hz=float('nan')), text=b'pll_bw_hz')
    plan(c=cfg(tap_samples=3), text=b'chip')           # a chip is 2.002 samples at 2048
    # a state whose first window lies before first_sample
    plan(c=cfg(first_sample=412), text=b'before first_sample')
    plan(c=cfg(first_sample=411), want=0)
    s2 = st.copy()
    s2['tau'][3] = 0.5
    plan(st=s2, text=b'before first_sample')
    for field, bad in (('prn', 0), ('prn', 38), ('bit_no', -1), ('f_hz', float('nan')), ('tau', float('inf'))):
        s2 = st.copy()
        s2[field][3] = bad
        plan(st=s2, text=field.encode())
    plan(cs=4096, want=-5)


def test_open_from_a_refined_record():
    """gpsmi_wtrk_open against open_ref, on the records refinement's restatement gives for the deep
    scene, and on a hit below the tap spacing (which refinement counts from the next period)."""
    from gpsmi import _lib
    from gpsmi.acquisition import open_weak_channels
    from gpsmi.engine import Config
    _, states, rec = W.opened()
    r32 = np.zeros(5, _lib.REFINE_OUT_DTYPE)
    for name in r32.dtype.names:
        r32[name] = rec[name][:5]
    got = open_weak_channels(r32, Config(), data_start=7000)
    for g, r in zip(got, r32):
        want = W.open_ref(r, 2048, data_start=7000)
        assert g['prn'] == want['prn'] and g['tau'] == want['tau'] and g['bit_no'] == 0
        assert g['f_hz'] == g['f_acc'] == want['f_hz'] and g['theta'] == 0 and g['lock'] == 0
        assert not g['mu_ring'].any()
    near = r32[:1].copy()
    near['code_phase'], near['edge_ms'], near['tap_metric'] = 0.2, 19, (5.0, 9.0, 6.0)
    g = open_weak_channels(near, Config())[0]
    Tc = 2048 / (1.0 + near['f_hz'][0] / L1_HZ)
    assert g['tau'] == 0.2 + 20.0 * Tc
    near['code_phase'] = -1.0
    with pytest.raises(_lib.EngineError, match=r'\(-1\)'):
        open_weak_channels(near, Config())


# ---- the option and shape cases of small_scene.py ----------------------------------------------------

@pytest.mark.parametrize('name', list(S.TRACK_CASES))
def test_small_scene_windows_keep_clear_of_integers(name):
    """As test_windows_keep_clear_of_integers, for every scene test_gpu_track_cases.py compares window
    by window: the restatement's s_k stay more than INTEGER_GUARD from an integer, in the far case at
    stream positions past 2^31 (where an ulp of tau is 4.8e-7)."""
    case = S.TRACK_CASES[name]
    rec, st, nk = case.ref(first_sample=S.FAR if name == 'far' else 0)
    assert [s['bit_no'] for s in st] == [case.n_bits] * len(st) and not any(s['flags'] for s in st)
    worst = S.closest_to_integer(rec, st, nk, case.cs, **case.scene_kw())
    print('%s: closest s_k to an integer: %.3e' % (name, worst))
    assert worst > INTEGER_GUARD
    if name == 'far':
        assert nk.min() > 2 ** 31


def test_small_scene_cases_reach_what_they_are_for():
    ring = S.TRACK_CASES['ring']
    rec, st, _ = ring.ref()
    assert ring.n_bits > W.RING and len(st) == 3 and st[2]['prn'] == 3
    assert not np.isnan(rec[:2, W.RING:]['cn0_dbhz']).any()          # the wrapped ring gives a C/N0
    many = S.TRACK_CASES['many']
    assert len(many.states()) == 64
    cut = S.many_cut(many)
    _, sc, _ = many.ref(n=cut)
    stopped = [s['bit_no'] for s in sc].count(2)
    assert 16 <= stopped <= 48 and stopped + [s['bit_no'] for s in sc].count(3) == 64
    assert all((s['flags'] == 1) == (s['bit_no'] == 2) for s in sc)
    for name in ('slide-minus-2048', 'slide-plus-16368'):                # windows sliding samples per ms
        c = S.TRACK_CASES[name]
        _, _, nk = c.ref()
        step = np.diff(nk[0, 0]) - c.cs
        assert np.all(np.abs(step) >= 3) and np.all((step > 0) == (c.opts['f_offset'] > 0))
