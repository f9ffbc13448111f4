"""Float64 numpy restatement of the spatial signatures (gpsmi_acq_signature, include/gpsmi.h;
DESIGN.md 4.2p), shared by test_signature.py and test_snapshot_signature.py (CPU), test_gpu_signature.py
and test_gpu_snapshot_signature.py (GPU), and the scenes they run on.

One record (prn, f_hz, tau) over the rows x[a][n] of A antennas: Tc = cs / (1 + (f_hz - f_offset) /
carrier_hz), j_k = rint(tau + k Tc); its windows are all k with 0 <= j_k and j_k + cs <= n, in order, of
which a positive n_ms keeps the first n_ms.  Prompts P[a][k] = sum_i x[a][j_k + i]
exp(-i 2 pi f_hz (j_k + i + 1) / fs) replica[i]; covariance C[a][b] = sum_k P[a][k] conj(P[b][k])."""
import functools

import numpy as np

from cancel_ref import L1_HZ, replica64


def sig_windows(n, cs, f_hz, tau, n_ms=0, carrier_hz=L1_HZ, f_offset=0.0):
    """The window starts j_k of one record inside [0, n), in order."""
    Tc = cs / (1.0 + (f_hz - f_offset) / carrier_hz)

    def j(k):
        return int(np.rint(tau + float(k) * Tc))

    k = int(np.floor(-tau / Tc))
    while j(k) >= 0:
        k -= 1
    while j(k) < 0:
        k += 1
    out = []
    while j(k) + cs <= n and not (n_ms > 0 and len(out) >= n_ms):
        out.append(j(k))
        k += 1
    return out


def sig_ref(x, sats, cs, n_ms=0, carrier_hz=L1_HZ, f_offset=0.0):
    """x: [A][n] samples (any complex, or the decoded raw ones); sats: [(prn, f_hz, tau)].
    -> (prompts complex128 [R][A][max_windows], zero past a record's last window; cov complex128
    [R][A][A]; n_win int32 [R])."""
    x = np.asarray(x).astype(np.complex128)
    A, n = x.shape
    fs = 1000.0 * cs
    wins = [sig_windows(n, cs, f, tau, n_ms, carrier_hz, f_offset) for _, f, tau in sats]
    max_w = max(len(w) for w in wins)
    P = np.zeros((len(sats), A, max_w), np.complex128)
    i = np.arange(cs, dtype=np.float64)
    for r, (prn, f, _) in enumerate(sats):
        rep = replica64(prn, cs)
        for k, j in enumerate(wins[r]):
            w = np.exp(-2j * np.pi * np.mod(f * (j + i + 1.0) / fs, 1.0)) * rep
            P[r, :, k] = x[:, j:j + cs] @ w
    C = np.einsum('rak,rbk->rab', P, P.conj())
    return P, C, np.array([len(w) for w in wins], np.int32)


# ---- the scenes ---------------------------------------------------------------------------------
KERNEL_N = {2048: 6 * 2048 + 123, 16368: 130944}
KERNEL_ANTENNAS = {2048: (2, 3, 8), 16368: (2, 4)}
KERNEL_SINES = (-0.7, 0.2, 0.85, -0.1)


def kernel_sats(cs):
    """(prn, Doppler, delay) of the kernel scene: a code start within a sample of 0, one just below
    cs, one in mid-period, and PRN 4 a second time at another code start."""
    k = cs / 2048.0
    return ((4, 3094.0, 0.3), (5, -4321.0, cs - 0.4), (9, 400.0, 1347.4 * k), (4, 3090.0, 700.2 * k))


def kernel_records(cs):
    """The records of one call: both Doppler signs, tau within a sample of 0, just below cs,
    negative, and the same PRN twice."""
    k = cs / 2048.0
    return [(4, 3096.0, 0.3), (5, -4319.0, cs - 0.3), (9, 402.0, 1347.4 * k - cs), (4, 3091.0, 700.2 * k)]


@functools.lru_cache(maxsize=None)
def kernel_raw(cs):
    """uint16 [8 or 4][n]: the kernel scene as every antenna's recorder wrote it, read-only; the
    first A rows serve a call over A antennas."""
    from gpsmi import synth, synth_array
    sats = [synth.Sat(prn=p, doppler=f, delay=d, amp=0.11, phase0=0.4 * i) for i, (p, f, d) in enumerate(kernel_sats(cs))]
    sc = synth.Scene(sats=sats, seed=31, noise_sigma=0.35, code_samples=cs, n_cyc=32 if cs == 2048 else 8)
    arr = synth_array.ArrayScene(sc, synth_array.ula_steering(max(KERNEL_ANTENNAS[cs]), KERNEL_SINES))
    out = arr.block_raw(0, n=KERNEL_N[cs])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kernel_c64(cs):
    from gpsmi.synth import raw_to_c64
    out = raw_to_c64(kernel_raw(cs))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kernel_reference(cs, A, n_ms=0):
    return sig_ref(kernel_c64(cs)[:A], kernel_records(cs), cs, n_ms)


# the spoofed scene of spoof_truth.py seen by four antennas: a uniform line, the eight authentic
# satellites at the sines -0.875 + 0.25 i, everything the spoofer adds at the sine 0.3
SNAP_ANTENNAS = 4
AUTHENTIC_SINES = tuple(-0.875 + 0.25 * i for i in range(8))
SPOOFER_SINE = 0.3
SIG_MS = 64                      # the span the CPU tests take their signatures over


def snapshot_array(which):
    """The ArrayScene of 'spoofed' (spoof_truth.spoofed), 'clean' (snapshot_truth.strong) or
    'spoofer' (the spoofed scene with the authentic amplitudes 0), unit scale: antenna 0 is the
    single-antenna scene itself."""
    from dataclasses import replace

    import snapshot_truth as T
    import spoof_truth as ST
    from gpsmi import synth_array
    if which == 'clean':
        sc = T.strong()[0]
    else:
        sc = ST.spoofed()[0]
        if which == 'spoofer':
            sc = replace(sc, sats=[replace(s, amp=0.0) for s in sc.sats[:8]] + list(sc.sats[8:]), _rep=sc._rep)
    sines = list(AUTHENTIC_SINES) + [SPOOFER_SINE] * (len(sc.sats) - 8)
    return synth_array.ArrayScene(sc, synth_array.ula_steering(SNAP_ANTENNAS, sines), scale=1.0)


@functools.lru_cache(maxsize=None)
def snapshot_raw(which, n_ms=None):
    """uint16 [4][n] of snapshot_array(which), read-only: the first n_ms milliseconds (None: the
    whole second), rendered in pieces of eight blocks."""
    import snapshot_truth as T
    arr = snapshot_array(which)
    cs = arr.scene.code_samples
    n = (int(round(T.STRONG_SECONDS * 1000)) if n_ms is None else n_ms) * cs
    step = 8 * arr.ngps
    out = np.concatenate([arr.block_raw(k // arr.ngps, n=min(step, n - k)) for k in range(0, n, step)], axis=1)
    out.setflags(write=False)
    return out

