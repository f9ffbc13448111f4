"""Numpy restatement of the auxiliary peaks (gpsmi_acq_peaks_dev, include/gpsmi.h),
shared by test_peaks.py (CPU) and test_gpu_peaks.py (GPU).

Step a: float32 throughout, every operation rounded on its own; mean and std are collective_ref's
row_stats (the kernels share one device function, the restatements one Python function).  Step b: k
times the first index of the maximum of zmax among the free lags, then the stripe of the guard is
taken.  The same inputs give the same bytes as the kernels."""
import numpy as np

from collective_ref import row_stats

PICK_DTYPE = np.dtype([('lag', np.int32), ('bin', np.int32), ('z', np.float32), ('s', np.float32)])


def default_guard(cs):
    """Two chips in samples: 4 at 2048, 32 at 16368."""
    return 4 if cs == 2048 else 32


def surface_z(S, lo, hi):
    """z float32 [nbins][cs] of one satellite's surfaces (0 outside the window and in skipped bins)
    and which bins of the window are not skipped."""
    S = np.asarray(S, np.float32)
    z = np.zeros(S.shape, np.float32)
    used = np.zeros(S.shape[0], bool)
    for b in range(lo, hi + 1):
        mean, sd = row_stats(S[b])
        if not sd > 0:
            continue
        z[b] = (S[b] - mean) / sd
        used[b] = True
    return z, used


def peaks_one(S, k=4, guard=-1, bins=None):
    """One satellite: S float32 [nbins][cs] -> (picks PICK_DTYPE [k], cols float32 [k][2][nbins])."""
    S = np.asarray(S, np.float32)
    lo, hi = (0, S.shape[0] - 1) if bins is None else bins
    return picks_of(S, *surface_z(S, lo, hi), k, guard)


def picks_of(S, z, used, k=4, guard=-1):
    """Step b on surface_z's result (a test that sweeps k and the guard forms z once)."""
    nbins, cs = S.shape
    guard = default_guard(cs) if guard < 0 else guard
    picks = np.zeros(k, PICK_DTYPE)
    picks['lag'] = picks['bin'] = -1
    cols = np.zeros((k, 2, nbins), np.float32)
    if not used.any():
        return picks, cols
    ub = np.flatnonzero(used)
    zmax = z[ub].max(axis=0)
    zbin = ub[np.argmax(z[ub], axis=0)]                   # (the first, hence the smallest, bin of equal ones)
    free = np.ones(cs, bool)
    lags = np.arange(cs)
    for i in range(k):
        if not free.any():
            break
        cand = np.where(free, zmax, -np.inf)
        lag = int(np.flatnonzero(free & (cand == cand[free].max()))[0])
        b = int(zbin[lag])
        picks[i] = (lag, b, zmax[lag], S[b, lag])
        cols[i, 0] = S[:, lag]
        cols[i, 1] = z[:, lag]
        d = np.abs(lags - lag)
        free &= np.minimum(d, cs - d) > guard
    return picks, cols


def peaks(rows, k=4, guard=-1, bins=None):
    """rows float32 [nsv][nbins][cs] -> (picks [nsv][k], cols [nsv][k][2][nbins])."""
    out = [peaks_one(S, k, guard, bins) for S in rows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def column_bin(col, corr_min):
    """largest_peak_hits' rule on a pick's columns: among the bins with z > corr_min at the pick's
    lag the one of largest S, first index; -1 where none passes."""
    ok = col[1] > corr_min
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, col[0], -np.inf)))
