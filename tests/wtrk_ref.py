"""Float64 numpy restatement of the bit-synchronous tracking of refined hits (gpsmi_acq_track,
include/gpsmi.h), shared by test_acq_track.py (CPU) and test_gpu_acq_track.py (GPU), the scenes
both run, and the bounds on the truth both assert.

Per bit of a state (tau, f, theta): Tc = cs / (1 + (f - f_offset) / carrier), s_k = tau + k Tc,
n_k = floor(s_k), a_k = s_k - n_k; whole-sample sums D[o][sh][k] = sum_i x c R[(i - sh) mod cs] at
o = -tap, 0, +tap, blended a_k D[o][1] + (1 - a_k) D[o][0]; the carrier phase is a 64-bit integer
(Python / uint64 arithmetic here) whose top 24 bits give the angle; one loop update per bit.  The
only things the device does differently are the float32 sample sums and its own libm."""
import functools
import math

import numpy as np

from deep_ref import DEEP_HIGH, DEEP_ZERO, L1_HZ, deep_scene
from refine_ref import ABSENT, refine_ref, scene_cases

RING = 50
T = 0.020
LOCK_ALPHA = 0.05
DEF_PLL, DEF_FLL, DEF_DLL, DEF_PULL_IN = 4.0, 1.0, 0.5, 10
M64 = (1 << 64) - 1

BIT_DTYPE = np.dtype([
    ('p_i', np.float64), ('p_q', np.float64), ('abs_e', np.float64), ('abs_l', np.float64),
    ('h0_i', np.float64), ('h0_q', np.float64), ('h1_i', np.float64), ('h1_q', np.float64),
    ('f_hz', np.float64), ('tau', np.float64), ('cn0_dbhz', np.float64), ('lock', np.float64),
    ('dll_err', np.float64), ('bit_no', np.int32)])


def default_tap(cs):
    return 1 if cs == 2048 else 8


def new_state(prn, tau, f_hz):
    return dict(prn=int(prn), bit_no=0, tau=float(tau), f_hz=float(f_hz), theta=0, f_acc=float(f_hz),
                lock=0.0, flags=0, mu_ring=[0.0] * RING)


def open_ref(rec, cs, data_start=0, refine_tap=0, carrier_hz=L1_HZ, f_offset=0.0):
    """gpsmi_wtrk_open on one record of refinement (any dtype with its field names)."""
    tap = refine_tap or default_tap(cs)
    E, P, L = (float(v) for v in rec['tap_metric'])
    den = E - 2.0 * P + L
    v = 0.5 * (E - L) / den * tap if den != 0.0 else 0.0
    delay = np.rint(float(rec['code_phase']) - v)
    Tc = cs / (1.0 + (float(rec['f_hz']) - f_offset) / carrier_hz)
    e = int(rec['edge_ms']) + (1 if delay < tap else 0)
    return new_state(rec['prn'], float(data_start) + float(rec['code_phase']) + float(e) * Tc, rec['f_hz'])


def gains(pll_bw=0.0, fll_bw=0.0, dll_bw=0.0):
    pll = DEF_PLL if pll_bw == 0.0 else pll_bw
    fll = DEF_FLL if fll_bw == 0.0 else fll_bw
    dll = DEF_DLL if dll_bw == 0.0 else dll_bw
    wp = pll / 0.53 if pll > 0.0 else 0.0
    wf = fll / 0.25 if fll > 0.0 else 0.0
    return wp * wp * T, 1.414 * wp, wf * T, 4.0 * dll * T


def phase_inc(f, fs):
    x = f / fs
    x -= math.floor(x)
    if not x < 1.0:
        x = 0.0
    return int(x * 2.0 ** 64)


def windows(tau, f, cs, carrier_hz=L1_HZ, f_offset=0.0):
    """(Tc, s_k, n_k) of the bit that starts at (tau, f): float64, one operation per rounding."""
    Tc = cs / (1.0 + (f - f_offset) / carrier_hz)
    s = tau + np.arange(20, dtype=np.float64) * Tc
    return Tc, s, np.floor(s).astype(np.int64)


def track_ref(data, states, n_bits, cs, first_sample=0, tap=0, pll_bw=0.0, fll_bw=0.0, dll_bw=0.0,
              pull_in_bits=0, carrier_hz=L1_HZ, f_offset=0.0):
    """-> (records BIT_DTYPE [nhits, n_bits], states, n_k int64 [nhits, n_bits, 20]); the records
    past a channel's last bit are zero."""
    from gpsmi import codes
    tap = tap or default_tap(cs)
    x = np.asarray(data).astype(np.complex128)
    n, fs = len(x), 1000.0 * cs
    k_p1, k_p2, k_f, k_d = gains(pll_bw, fll_bw, dll_bw)
    pull_in = DEF_PULL_IN if pull_in_bits == 0 else max(pull_in_bits, 0)
    cmt = cs / 1023.0 - tap
    out = np.zeros((len(states), n_bits), BIT_DTYPE)
    nks = np.zeros((len(states), n_bits, 20), np.int64)
    res = []
    i = np.arange(cs, dtype=np.int64)
    for h, st0 in enumerate(states):
        st = dict(st0, mu_ring=list(st0['mu_ring']))
        st['flags'] = 0
        R = codes.code_replica(st['prn'], cs).astype(np.float32).astype(np.float64)
        R1 = np.roll(R, 1)                                   # R[(i - 1) mod cs]
        for b in range(n_bits):
            tau, f = st['tau'], st['f_hz']
            Tc, s, nk = windows(tau, f, cs, carrier_hz, f_offset)
            lo, hi = min(nk[0], nk[19]) - tap, max(nk[0], nk[19]) + cs + tap
            if not (math.isfinite(Tc) and lo >= first_sample and hi <= first_sample + n):
                st['flags'] = 1
                break
            a = s - nk
            nks[h, b] = nk
            inc = phase_inc(f, fs)
            j = np.arange(lo, hi, dtype=np.int64)
            ph = (np.uint64(st['theta']) + (j - nk[0]).astype(np.uint64) * np.uint64(inc))
            ang = (ph.astype(np.int64) >> np.int64(40)).astype(np.float64) * 2.0 ** -23
            y = x[lo - first_sample:hi - first_sample] * np.exp(-1j * np.pi * ang)
            z = np.zeros((3, 20), np.complex128)
            for t, o in enumerate((-tap, 0, tap)):
                idx = (nk + o - lo)[:, None] + i[None, :]
                seg = y[idx]
                z[t] = a * (seg @ R1) + (1.0 - a) * (seg @ R)
            E, L = z[0].sum(), z[2].sum()
            h0, h1 = z[1, :10].sum(), z[1, 10:].sum()
            P = h0 + h1
            w = float((np.abs(z[1]) ** 2).sum())
            ae, al, pp = abs(E), abs(L), P.real * P.real + P.imag * P.imag
            e_f = math.atan2(h0.real * h1.imag - h0.imag * h1.real,
                             h0.real * h1.real + h0.imag * h1.imag) / (2.0 * math.pi * 0.010)
            if P.real == 0.0:
                e_p = 0.25 * np.sign(P.imag)
            else:
                e_p = math.atan(P.imag / P.real) / (2.0 * math.pi)
            e_d = cmt * (al - ae) / (ae + al) if ae + al > 0.0 else 0.0
            bn = st['bit_no']
            st['mu_ring'][bn % RING] = float(np.float32(pp / w if w > 0.0 else 0.0))
            cnt = min(bn + 1, RING)
            mu = sum(st['mu_ring'][:cnt]) / cnt
            st['lock'] += LOCK_ALPHA * ((((P.real * P.real - P.imag * P.imag) / pp) if pp > 0.0 else 0.0) - st['lock'])
            cn0 = 10.0 * math.log10(1000.0 * (mu - 1.0) / (20.0 - mu)) if mu > 1.0 else math.nan
            out[h, b] = (P.real, P.imag, ae, al, h0.real, h0.imag, h1.real, h1.imag, f, tau, cn0,
                         st['lock'], e_d, bn)
            ep = e_p if (k_p2 > 0.0 and bn >= pull_in) else 0.0
            ef = e_f if k_f > 0.0 else 0.0
            st['f_acc'] += k_p1 * ep + k_f * ef
            st['f_hz'] = st['f_acc'] + k_p2 * ep
            tau1 = (tau + 20.0 * Tc) + k_d * e_d
            dn = int(math.floor(tau1) - math.floor(tau))
            st['theta'] = (st['theta'] + dn * inc) & M64
            st['tau'] = tau1
            st['bit_no'] = bn + 1
        res.append(st)
    return out, res, nks


def states_array(states):
    """The dict states as the binding's WTRK_STATE_DTYPE array."""
    from gpsmi._lib import WTRK_STATE_DTYPE
    a = np.zeros(len(states), WTRK_STATE_DTYPE)
    for i, s in enumerate(states):
        a[i] = (s['prn'], s['bit_no'], s['tau'], s['f_hz'], s['theta'], s['f_acc'], s['lock'],
                s['flags'], 0, s['mu_ring'])
    return a


def weak_bits_ref(rec):
    p = rec['p_i'] + 1j * rec['p_q']
    return np.where(p.real >= 0, 1, -1), np.where((p[..., 1:] * np.conj(p[..., :-1])).real >= 0, 1, -1)


# ---- truth of a deep_scene ------------------------------------------------------------------------

def truth_of(scene, prn):
    return next(s for s in scene.sats if s.prn == prn)


def tau_error(scene, prn, tau):
    """tau minus the nearest true code start, samples (synth: code starts where
    k - (delay + rate k) is a multiple of cs, rate = -doppler / L1)."""
    s = truth_of(scene, prn)
    cs = scene.code_samples
    pos = np.asarray(tau) * (1.0 + s.doppler / L1_HZ) - s.delay
    return (pos + cs / 2.0) % cs - cs / 2.0


def true_bits(scene, prn, tau):
    """synth's data bit (+-1) of the code period that starts nearest tau."""
    from gpsmi.synth import _mix64
    s = truth_of(scene, prn)
    cs = scene.code_samples
    period = np.rint((np.asarray(tau) * (1.0 + s.doppler / L1_HZ) - s.delay) / cs).astype(np.int64)
    bit_no = np.floor(period / 20.0).astype(np.int64)
    h = _mix64((bit_no + (1 << 40)).astype(np.uint64) ^ np.uint64(scene.seed * 1000 + prn))
    return 1 - 2 * (h & np.uint64(1)).astype(np.int64)


# ---- the scenes -------------------------------------------------------------------------------------

N_BLOCKS = 33
N_BITS = 45
REFINE_MS = 1000
# the strong scene: deep_scene with the amplitude raised by 9.5 dB (amp^2 fs / sigma^2 = 35.0 dB-Hz)
STRONG_AMP = 0.0046 * 10.0 ** (9.5 / 20.0)
HIRATE_MS, HIRATE_BITS = 300, 12


@functools.lru_cache(maxsize=None)
def scene_raw(amp=None, cs=2048):
    sc = deep_scene(cs, 32 if cs == 2048 else 8, **({} if amp is None else {'amp': amp}))
    n = N_BLOCKS * 65536 if cs == 2048 else (HIRATE_MS + 2) * cs + 8
    raw = sc.block_raw(0, n=n)
    raw.setflags(write=False)
    return raw


def scene_c64(amp=None, cs=2048):
    from gpsmi.synth import raw_to_c64
    return raw_to_c64(scene_raw(amp, cs))


@functools.lru_cache(maxsize=None)
def opened(amp=None, cs=2048):
    """The channels of a scene as the hand-over gives them: refinement's restatement on the same
    data (case A: the five satellites and the absent candidate), opened by open_ref.
    -> (scene, states, refined records)."""
    sc = deep_scene(cs, 32 if cs == 2048 else 8, **({} if amp is None else {'amp': amp}))
    n_ms = REFINE_MS if cs == 2048 else HIRATE_MS
    _, hits, _ = scene_cases(sc, n_ms, cs)['A']
    rec, _, _ = refine_ref(scene_c64(amp, cs), hits, n_ms, cs)
    states = []
    for r in rec:
        if r['code_phase'] < 0:                      # (the absent candidate may have no vertex)
            r = r.copy()
            r['code_phase'] = float(hits[len(states)][2])
            r['tap_metric'] = (0.0, 1.0, 0.0)
        states.append(open_ref(r, cs))
    return sc, states, rec


@functools.lru_cache(maxsize=None)
def tracked(amp=None, cs=2048):
    """The restatement's run over a scene, computed once: (records, states, n_k)."""
    sc, states, _ = opened(amp, cs)
    n_bits = N_BITS if cs == 2048 else HIRATE_BITS
    return track_ref(scene_c64(amp, cs), states, n_bits, cs)
