"""Float64 numpy restatement of the refinement of weak / deep hits (gpsmi_acq_refine,
include/gpsmi.h), shared by test_acq_refine.py (CPU) and test_gpu_acq_refine.py (GPU), and the
cases both run on the pinned deep scene (deep_ref.py).

Stage 1: P[tau][k] = sum_i x[n_k + tau + i] exp(-j 2 pi f (n_k + tau + i) / fs) replica[i],
n_k = k cs + delay + rint(-(f - f_offset) / carrier * k * cs), tau = -tap, 0, +tap.
Stage 2: M[d][e] = sum_b |sum_{k = e + 20 b}^{e + 20 b + 19} P[0][k] exp(-j 2 pi df_d k / 1000)|^2."""
import numpy as np

from deep_ref import DEEP_HIGH, DEEP_ZERO, L1_HZ, nearest_bin

REFINE_DTYPE = np.dtype([
    ('prn', np.int32), ('edge_ms', np.int32), ('n_bits', np.int32), ('confirmed', np.int32),
    ('f_hz', np.float64), ('code_phase', np.float64), ('peak', np.float64), ('median', np.float64),
    ('ratio', np.float64), ('mu', np.float64), ('cn0_dbhz', np.float64),
    ('tap_metric', np.float64, (3,))])

ABSENT = (3, 1000.0, 100)            # a candidate that is not in the scene
CUT_MS = 7                           # case B: the data from sample CUT_MS * cs on


def default_tap(cs):
    return 1 if cs == 2048 else 8


def refine_prompts(data, hits, n_ms, cs, tap=None, carrier_hz=L1_HZ, f_offset=0.0):
    """complex128 [nhits, 3, n_ms]: early, prompt, late."""
    from gpsmi import codes
    tap = tap or default_tap(cs)
    x = np.asarray(data).astype(np.complex128)
    fs = 1000.0 * cs
    k = np.arange(n_ms, dtype=np.float64)
    i = np.arange(cs, dtype=np.int64)
    P = np.zeros((len(hits), 3, n_ms), np.complex128)
    for h, (prn, freq, delay) in enumerate(hits):
        rep = codes.code_replica(int(prn), cs)
        d0 = int(delay) + cs if delay < tap else int(delay)
        m = np.rint(-(freq - f_offset) / carrier_hz * k * cs).astype(np.int64)
        nk = np.arange(n_ms, dtype=np.int64) * cs + d0 + m
        lo, hi = int(nk.min()) - tap, int(nk.max()) + cs + tap
        assert lo >= 0 and hi <= len(x)
        j = np.arange(lo, hi, dtype=np.float64)
        y = x[lo:hi] * np.exp(-2j * np.pi * np.mod(freq * j / fs, 1.0))
        for t, tau in enumerate((-tap, 0, tap)):
            idx = (nk + tau - lo)[:, None] + i[None, :]
            P[h, t] = y[idx] @ rep
    return P


def bit_sums(p, df, e, B):
    """The B coherent 20-ms sums of the prompt row p from millisecond e on, derotated by df."""
    k = np.arange(len(p), dtype=np.float64)
    z = p * np.exp(-2j * np.pi * df * k / 1000.0)
    return z[e:e + 20 * B].reshape(B, 20).sum(axis=1)


def refine_grid(p0, dfs):
    """float64 [n_df, 20] of one prompt row."""
    n_ms = len(p0)
    B = n_ms // 20 - 1
    k = np.arange(n_ms, dtype=np.float64)
    z = p0[None, :] * np.exp(-2j * np.pi * np.asarray(dfs)[:, None] * k[None, :] / 1000.0)
    M = np.zeros((len(dfs), 20))
    for e in range(20):
        s = z[:, e:e + 20 * B].reshape(len(dfs), B, 20).sum(axis=2)
        M[:, e] = (np.abs(s) ** 2).sum(axis=1)
    return M


def refine_ref(data, hits, n_ms, cs, df_step=2.0, df_half=120.0, tap=None, carrier_hz=L1_HZ,
               f_offset=0.0, min_ratio=2.5):
    """-> (records REFINE_DTYPE [nhits], grid [nhits, n_df, 20], prompts [nhits, 3, n_ms])."""
    tap = tap or default_tap(cs)
    n_df = int(np.floor(2.0 * df_half / df_step + 1e-9)) + 1
    dfs = -df_half + np.arange(n_df, dtype=np.float64) * df_step
    B = n_ms // 20 - 1
    P = refine_prompts(data, hits, n_ms, cs, tap, carrier_hz, f_offset)
    grid = np.zeros((len(hits), n_df, 20))
    out = np.zeros(len(hits), REFINE_DTYPE)
    for h, (prn, freq, delay) in enumerate(hits):
        M = grid[h] = refine_grid(P[h, 1], dfs)
        best = int(np.argmax(M))                       # first index, (d, e) order
        d, e = divmod(best, 20)
        peak = M[d, e]
        median = np.sort(M.ravel())[(M.size - 1) // 2]
        f = freq + dfs[d]
        if 0 < d < n_df - 1:
            l, r = M[d - 1, e], M[d + 1, e]
            den = l - 2.0 * peak + r
            if den != 0.0:
                f += 0.5 * (l - r) / den * df_step
        tm = np.array([(np.abs(bit_sums(P[h, t], dfs[d], e, B)) ** 2).sum() for t in range(3)])
        if tm[0] > tm[1] or tm[2] > tm[1]:
            cp = -1.0
        else:
            den = tm[0] - 2.0 * tm[1] + tm[2]
            cp = delay + (0.5 * (tm[0] - tm[2]) / den * tap if den != 0.0 else 0.0)
        nb = np.abs(bit_sums(P[h, 1], dfs[d], e, B)) ** 2
        wb = (np.abs(P[h, 1, e:e + 20 * B]) ** 2).reshape(B, 20).sum(axis=1)
        mu = float(np.mean(np.divide(nb, wb, out=np.zeros_like(nb), where=wb > 0)))
        cn0 = 10.0 * np.log10(1000.0 * (mu - 1.0) / (20.0 - mu)) if mu > 1.0 else np.nan
        out[h] = (prn, e, B, int(peak / median > min_ratio), f, cp, peak, median, peak / median,
                  mu, cn0, tm)
    return out, grid, P


# ---- the cases on the deep scene ----------------------------------------------------------------

def scene_cases(scene, n_ms, cs):
    """Cases A (the data as it is) and B (from sample CUT_MS * cs on) of a deep_scene: per case
    (first sample, hits, truth), hits = the scene's satellites at (prn, nearest 200-Hz bin, true
    delay at the start of the data) plus the absent candidate; truth = per satellite (doppler,
    delay at the start of the data as a float, edge)."""
    k = cs / 2048.0
    sats = [(p, f, float(np.floor(d * k))) for p, f, d in DEEP_HIGH + [DEEP_ZERO]]
    cases = {}
    for name, cut in (('A', 0), ('B', CUT_MS)):
        hits, truth = [], []
        for p, f, d in sats:
            d_cut = (d - f / L1_HZ * cut * cs) % cs          # synth: delay + delay_rate * sample
            hits.append((p, nearest_bin(f), int(np.rint(d_cut)) % cs))
            truth.append((f, d_cut, (20 - cut) % 20))
        hits.append((ABSENT[0], ABSENT[1], int(np.floor(ABSENT[2] * k))))
        cases[name] = (cut * cs, hits, truth)
    return cases


def check_truth(rec, truth, cn0_band=(22.0, 26.0)):
    """The bounds of the issue on the records of one case (five satellites, then the absent
    candidate): every figure is printed before it is asserted."""
    for r, (dop, delay, edge) in zip(rec[:len(truth)], truth):
        print('prn %2d  edge %2d (%2d)  f_hz %+9.2f (err %+5.2f)  ratio %5.2f  cn0 %5.2f  '
              'code_phase %8.3f (err %+5.3f)' % (r['prn'], r['edge_ms'], edge, r['f_hz'],
                                                 r['f_hz'] - dop, r['ratio'], r['cn0_dbhz'],
                                                 r['code_phase'], r['code_phase'] - delay))
    a = rec[len(truth)]
    print('absent prn %d ratio %.3f' % (a['prn'], a['ratio']))
    for r, (dop, delay, edge) in zip(rec[:len(truth)], truth):
        assert r['edge_ms'] == edge
        assert abs(r['f_hz'] - dop) <= 6.0
        assert r['ratio'] > 3.1 and r['confirmed'] == 1
        assert cn0_band[0] <= r['cn0_dbhz'] <= cn0_band[1]
        assert abs(r['code_phase'] - delay) <= 0.5
    assert a['ratio'] < 1.9 and a['confirmed'] == 0
