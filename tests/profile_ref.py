"""Float64 numpy restatement of the multi-tap correlation profiles (gpsmi_acq_profile, include/gpsmi.h;
DESIGN.md 4.2r), shared by test_profile.py (CPU), test_gpu_profile.py and test_gpu_snapshot_profile.py
(GPU), and the small scenes the kernel cases run on.

One record (prn, skip_ms, f_hz, tau) on the samples x[n]: Tc = cs / (1 + (f_hz - f_offset) /
carrier_hz), j_k = rint(tau + k Tc); its windows are all k with j_k - Lh >= 0 and j_k + Lh + cs <= n, in
order; the first skip_ms are dropped, the rest cut into runs of coh_ms, an incomplete last run dropped,
a positive n_runs keeps the first n_runs.  w[u] = x[u] exp(-i pi a[u]) with a[u] the top 24 bits of
(u + 1) inc mod 2^64 as a signed fraction of pi (inc = f_hz / fs in 0.64 fixed point): the quantised
integer carrier of the kernels.  D[l][k] = sum_i w[j_k + l + i] replica[i], l = -Lh .. Lh; S[l][m] = the
sum of D[l][.] over run m, rounded to complex64; Q[l][l'] = sum_m S[l][m] conj(S[l'][m])."""
import functools

import numpy as np

from cancel_ref import L1_HZ, replica64
MAX_COH = 20


def phase_inc(f, fs):
    """f / fs mod 1 in 0.64 fixed point (ref_phase_inc of the kernels' host code)."""
    x = f / fs
    x -= np.floor(x)
    return int(x * 2.0 ** 64) if x < 1.0 else 0


def default_half(cs):
    return 8 if cs == 2048 else 32


def prof_windows(n, cs, f_hz, tau, Lh, skip_ms=0, coh_ms=MAX_COH, n_runs=0, carrier_hz=L1_HZ, f_offset=0.0):
    """The window starts j_k of one record's runs, int64 [runs][coh_ms] (no run: [0][coh_ms])."""
    Tc = cs / (1.0 + (f_hz - f_offset) / carrier_hz)

    def j(k):
        return int(np.rint(tau + float(k) * Tc))

    k = int(np.floor((Lh - tau) / Tc))
    while j(k) >= Lh:
        k -= 1
    while j(k) < Lh:
        k += 1
    k += skip_ms
    out = []
    while j(k) + cs + Lh <= n and not (n_runs > 0 and len(out) >= n_runs * coh_ms):
        out.append(j(k))
        k += 1
    runs = len(out) // coh_ms
    return np.array(out[:runs * coh_ms], np.int64).reshape(runs, coh_ms)


def carrier_angle(lo, hi, f_hz, fs):
    """a[u], u = lo .. hi - 1: the quantised phase of sample u as a fraction of pi in [-1, 1)."""
    inc = np.uint64(phase_inc(f_hz, fs))
    ph = (np.arange(lo, hi, dtype=np.int64) + 1).astype(np.uint64) * inc
    return (ph.view(np.int64) >> np.int64(40)).astype(np.float64) * 2.0 ** -23


def _taps(w, R, cs, K):
    """D[l] = sum_i w[l + i] R[i], l = 0 .. K - 1, of the wiped samples w[cs + K - 1]."""
    return np.lib.stride_tricks.sliding_window_view(w, cs)[:K] @ R


def prof_ref(x, sats, cs, half_taps=0, coh_ms=0, n_runs=0, carrier_hz=L1_HZ, f_offset=0.0, plain32=False):
    """x: [n] samples (any complex, or the decoded raw ones); sats: [(prn, skip_ms, f_hz, tau)].
    -> (sums complex128 [R][K][max_runs], the complex64-rounded values, zero past a record's last run;
    cov complex128 [R][K][K]; n_runs int32 [R]).
    plain32: the same sums evaluated plainly in numpy float32 -- the carrier's sine and cosine, the
    wiped samples, the dot products (numpy's own order) and the sum over a run all in single
    precision -- the yardstick the kernel's tolerance is formed from; Q from those sums in float64."""
    Lh = half_taps or default_half(cs)
    coh = coh_ms or MAX_COH
    K, fs = 2 * Lh + 1, 1000.0 * cs
    n = len(x)
    x = np.asarray(x).astype(np.complex64 if plain32 else np.complex128)
    wins = [prof_windows(n, cs, f, tau, Lh, skip, coh, n_runs, carrier_hz, f_offset) for _, skip, f, tau in sats]
    assert all(len(w) for w in wins), 'a record has no run'
    max_r = max(len(w) for w in wins)
    S = np.zeros((len(sats), K, max_r), np.complex128)
    for r, (prn, _, f, _) in enumerate(sats):
        R = replica64(prn, cs)
        if plain32:
            R = R.astype(np.float32)
        for m, run in enumerate(wins[r]):
            D = np.zeros((coh, K), x.dtype)
            for q, j in enumerate(run):
                a = np.pi * carrier_angle(j - Lh, j + Lh + cs, f, fs)
                if plain32:
                    e = (np.cos(a).astype(np.float32) - 1j * np.sin(a).astype(np.float32)).astype(np.complex64)
                else:
                    e = np.exp(-1j * a)
                D[q] = _taps(x[j - Lh:j + Lh + cs] * e, R, cs, K)
            S[r, :, m] = (D.sum(axis=0) if plain32 else D.sum(axis=0).astype(np.complex64)).astype(np.complex128)
    Q = np.einsum('rlm,rkm->rlk', S, S.conj())
    return S, Q, np.array([len(w) for w in wins], np.int32)


def deviation(S, Q, S_ref, Q_ref):
    """(max |S - S_ref| / max |S_ref|, the largest over the records of max |Q - Q_ref| / trace Q_ref)."""
    d_s = np.abs(S - S_ref).max() / np.abs(S_ref).max()
    d_q = max(np.abs(Q[r] - Q_ref[r]).max() / np.trace(Q_ref[r]).real for r in range(len(Q_ref)))
    return d_s, d_q


# ---- the kernel scenes --------------------------------------------------------------------------
# 'short': the shapes of the signature's kernel scene (6 and 8 code periods); 'long' (2048 only): 45
# periods and an odd tail, which holds runs of 20 windows
KERNEL_N = {(2048, 'short'): 6 * 2048 + 123, (16368, 'short'): 130944, (2048, 'long'): 45 * 2048 + 57}
KERNEL_HALF = {2048: (1, 8, 32), 16368: (32, 5)}


def kernel_sats(cs):
    """(prn, Doppler, delay) of the kernel scene, as sig_ref's: a code start within a sample of 0, one
    just below cs, one in mid-period, and PRN 4 a second time half a chip or so behind the first --
    inside every profile of the first."""
    k = cs / 2048.0
    return ((4, 3094.0, 0.3), (5, -4321.0, cs - 0.4), (9, 400.0, 1347.4 * k), (4, 3094.0, 0.3 + 1.1 * k))


def kernel_records(cs, n, Lh, skip=(0, 7, 0, 0, 0)):
    """The records of one call: both Doppler signs; tau within a sample of 0 (its first windows fall
    away), just below cs, negative; PRN 4 twice; a record whose last window ends flush with n (Doppler
    0: Tc = cs exactly); skip_ms 0 and 7 (7 where the input holds more than 7 windows, else 1)."""
    k = cs / 2048.0
    windows = n // cs
    s = [v if windows > 8 else min(v, 1) for v in skip]
    flush = float(n - Lh - 3 * cs)                      # j = n - Lh - cs is a window start: it ends at n
    return [(4, s[0], 3096.0, 0.3), (5, s[1], -4319.0, cs - 0.3), (9, s[2], 402.0, 1347.4 * k - cs),
            (4, s[3], 3091.0, 700.2 * k), (11, s[4], 0.0, flush)]


@functools.lru_cache(maxsize=None)
def kernel_raw(cs, which='short'):
    """uint16 [n]: the kernel scene as the recorder wrote it, read-only."""
    from gpsmi import synth
    sats = [synth.Sat(prn=p, doppler=f, delay=d, amp=0.11, phase0=0.4 * i) for i, (p, f, d) in enumerate(kernel_sats(cs))]
    n = KERNEL_N[cs, which]
    sc = synth.Scene(sats=sats, seed=37, noise_sigma=0.35, code_samples=cs, n_cyc=64 if cs == 2048 else 8)
    out = sc.block_raw(0, n=n)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kernel_c64(cs, which='short'):
    from gpsmi.synth import raw_to_c64
    out = raw_to_c64(kernel_raw(cs, which))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kernel_reference(cs, which, Lh, coh_ms, n_runs=0, plain32=False):
    x = kernel_c64(cs, which)
    return prof_ref(x, kernel_records(cs, len(x), Lh), cs, Lh, coh_ms, n_runs, plain32=plain32)
