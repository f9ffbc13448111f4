"""Float64 numpy restatement of strong-satellite cancellation (gpsmi_acq_cancel, include/gpsmi.h;
DESIGN.md 4.2j), shared by test_cancel.py (CPU), test_gpu_cancel.py and test_gpu_snapshot_cancel.py
(GPU), and the scenes they run on.

One satellite (prn, f_hz, tau): Tc = cs / (1 + (f_hz - f_offset) / carrier_hz).  Window k holds the
samples ceil(tau + k Tc) <= n < ceil(tau + (k + 1) Tc) cut to [0, n_samples).  With
j = rint(tau + k Tc) the basis is b_d[n] = replica[(n - j - d) mod cs] exp(i 2 pi f_hz (n + 1) / fs),
d = -1, 0, +1; the window's samples are replaced by x - B c with G c = B^H x.  A window of fewer
than min_window samples, or whose smallest pivot of G (LDL^T, no permutation) is below
1e-6 trace(G), passes through.  Satellites one after another, each on the output of the one before."""
import numpy as np

L1_HZ = 1575.42e6
MIN_WINDOW = 16
PIVOT_MIN = 1.0e-6

CANCEL_DTYPE = np.dtype([('prn', np.int32), ('n_windows', np.int32), ('n_skipped', np.int32),
                         ('energy_in', np.float64), ('energy_removed', np.float64)])


def replica64(prn, cs):
    """The time-domain replica as the handle holds it: float32, here widened."""
    from gpsmi import codes
    return codes.code_replica(int(prn), cs).astype(np.float32).astype(np.float64)


def cancel_windows(n, cs, f_hz, tau, carrier_hz=L1_HZ, f_offset=0.0):
    """[(lo, hi, j)] of every window that holds a sample of [0, n), in order."""
    Tc = cs / (1.0 + (f_hz - f_offset) / carrier_hz)

    def edge(k):
        return tau + float(k) * Tc

    k = int(np.floor(-tau / Tc))
    while np.ceil(edge(k)) > 0:
        k -= 1
    while np.ceil(edge(k + 1)) <= 0:
        k += 1
    out = []
    while True:
        e0 = edge(k)
        lo, hi = int(np.ceil(e0)), int(np.ceil(edge(k + 1)))
        if lo >= n:
            break
        out.append((max(lo, 0), min(hi, n), int(np.rint(e0))))
        k += 1
    return out


def pivots(G):
    """The pivots of the LDL^T factorisation of a 3 x 3 Gram matrix, in order; a pivot that is
    not positive ends it (the remaining ones count as 0)."""
    d0 = G[0, 0]
    if not d0 > 0:
        return np.array([d0, 0.0, 0.0])
    l10, l20 = G[0, 1] / d0, G[0, 2] / d0
    d1 = G[1, 1] - l10 * G[0, 1]
    if not d1 > 0:
        return np.array([d0, d1, 0.0])
    l21 = (G[1, 2] - l20 * G[0, 1]) / d1
    d2 = G[2, 2] - l20 * G[0, 2] - l21 * l21 * d1
    return np.array([d0, d1, d2])


def cancel_ref(x, sats, cs, carrier_hz=L1_HZ, f_offset=0.0, min_window=MIN_WINDOW):
    """x: the samples (any complex or the decoded raw ones); sats: [(prn, f_hz, tau)].
    -> (y complex128 [n], records CANCEL_DTYPE [nsat], coef complex128 [nsat, max_windows, 3],
    processed bool [nsat, n]: the samples of the windows that were not skipped)."""
    y = np.asarray(x).astype(np.complex128).copy()
    n, fs = len(y), 1000.0 * cs
    wins = [cancel_windows(n, cs, f, tau, carrier_hz, f_offset) for _, f, tau in sats]
    max_w = max([len(w) for w in wins], default=0)
    rec = np.zeros(len(sats), CANCEL_DTYPE)
    coef = np.zeros((len(sats), max_w, 3), np.complex128)
    done = np.zeros((len(sats), n), bool)
    for s, (prn, f, tau) in enumerate(sats):
        rep = replica64(prn, cs)
        rec[s]['prn'], rec[s]['n_windows'] = prn, len(wins[s])
        for w, (lo, hi, j) in enumerate(wins[s]):
            nn = np.arange(lo, hi, dtype=np.int64)
            R = np.stack([rep[(nn - j - d) % cs] for d in (-1, 0, 1)], axis=1)
            G = R.T @ R
            if hi - lo < min_window or not pivots(G).min() >= PIVOT_MIN * np.trace(G):
                rec[s]['n_skipped'] += 1
                continue
            ph = np.exp(2j * np.pi * np.mod(f * (nn + 1.0) / fs, 1.0))
            B = R * ph[:, None]
            p = B.conj().T @ y[lo:hi]
            c = np.linalg.solve(G, p)
            rec[s]['energy_in'] += np.sum(np.abs(y[lo:hi]) ** 2)
            rec[s]['energy_removed'] += float((c.conj() @ G @ c).real)
            y[lo:hi] -= B @ c
            coef[s, w] = c
            done[s, lo:hi] = True
    return y, rec, coef, done


def residual_db(y, x_sat):
    """Power of what is left over the power of the satellite that was there, dB."""
    return 10.0 * np.log10(np.sum(np.abs(y) ** 2) / np.sum(np.abs(x_sat) ** 2))


# ---- the scenes ---------------------------------------------------------------------------------
DEPTH_AMP, DEPTH_MS = 0.11, 64
DEPTH_DOPPLERS = (3094.0, -4321.0)
# (frequency error Hz, code-start error samples, the residual the cancellation may leave, dB)
DEPTH_CASES = ((0.0, 0.0, -50.0), (3.0, 0.3, -40.0), (10.0, 0.45, -30.0))


def depth_scene(doppler, cs=2048, prn=7, delay=417.3, n_ms=DEPTH_MS):
    """One amplitude-0.11 satellite, noise-free and unquantised: (samples complex128, true tau)."""
    from gpsmi import synth
    sc = synth.Scene(sats=[synth.Sat(prn=prn, doppler=doppler, delay=delay * cs / 2048.0, amp=DEPTH_AMP,
                                     phase0=0.9)], seed=5, noise_sigma=0.0, code_samples=cs)
    x = sc.block_float(0, n=n_ms * cs)
    return x, delay * cs / 2048.0 / (1.0 + doppler / L1_HZ), prn


COLLISION_SEED, COLLISION_BLOCKS = 89, 16
COLLISION_STRONG = [(4, 400.0, 300.2), (5, -1276.0, 1500.7), (9, 2585.0, 900.5)]
COLLISION_WEAK = (3, 1402.0, 1200.4)
COLLISION_AMP = 0.00772                       # 30 dB-Hz; 0.01373 is 35, 0.0046 25.5
COLLISION_PRNS = [3, 4, 5, 9, 10, 31]
COLLISION_BIN = 1400.0


def collision_scene(weak_amp=COLLISION_AMP):
    """Three strong satellites and a weak one 2 Hz from PRN 4 modulo 1 kHz, default noise."""
    from gpsmi import synth
    sats = [synth.Sat(prn=p, doppler=f, delay=d, amp=0.11, phase0=0.5 * i)
            for i, (p, f, d) in enumerate(COLLISION_STRONG)]
    p, f, d = COLLISION_WEAK
    sats.append(synth.Sat(prn=p, doppler=f, delay=d, amp=weak_amp, phase0=1.3))
    return synth.Scene(sats=sats, seed=COLLISION_SEED, noise_sigma=0.35, code_samples=2048, n_cyc=32)


def collision_raw(weak_amp=COLLISION_AMP, blocks=COLLISION_BLOCKS):
    sc = collision_scene(weak_amp)
    return sc.block_raw(0, n=blocks * sc.ngps)


def true_tau(doppler, delay):
    """The first code start of a synth.Sat at or near sample 0, as a float."""
    return delay / (1.0 + doppler / L1_HZ)


def nc_surface(x, prn, f_bin, cs=2048, n_coh=4):
    """The non-coherent surface of one (PRN, bin): the mean over the n_coh-ms segments of |circular
    correlation of the folded, wiped-off segment with the replica|.  float64 [cs]."""
    x = np.asarray(x).astype(np.complex128)
    n_seg = len(x) // (n_coh * cs)
    n = n_seg * n_coh * cs
    k = np.arange(n, dtype=np.float64)
    seg_t = np.mod(k, n_coh * cs) + 1.0               # SEC_TIME restarts with every segment
    w = x[:n] * np.exp(-2j * np.pi * f_bin * seg_t / (1000.0 * cs))
    folded = w.reshape(n_seg, n_coh, cs).sum(axis=1)
    R = np.conj(np.fft.fft(replica64(prn, cs)))
    corr = np.fft.ifft(np.fft.fft(folded, axis=1) * R[None, :], axis=1)
    return np.abs(corr).mean(axis=0)


def norm_max_corr(surface):
    """(normMaxCorr, argmax) of a surface."""
    a = int(np.argmax(surface))
    return (surface[a] - surface.mean()) / surface.std(), a
