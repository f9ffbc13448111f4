"""Numpy restatement of collective detection (gpsmi_acq_collective_dev, include/gpsmi.h; DESIGN.md
4.2k), shared by test_collective.py (CPU) and test_gpu_collective.py (GPU).

Step a (normalise): float32 throughout, every operation rounded on its own.  The sums are formed as
the kernel forms them: share t of 256 adds lags t, t + 256, ... in ascending order from 0, the 256
shares meet in an adjacent-pair tree.  Step b (grid): float64 indices evaluated left to right,
float32 sums in ascending satellite order, the largest score per grid point, ties to the smallest
clock lag.  The same inputs give the same bytes as the kernels.

pyramid() restates the coarse-to-fine driver of gpsmi.snapshot.collective_pyramid on these
functions.  It shares the host geometry (snapshot.collective_model / collective_levels /
collective_level_args, which test_collective.py checks against finite differences of the range
model) and restates the loop: linearise, search a level, move to its best cell, halve."""
import numpy as np

SAT_DTYPE = np.dtype([('row', np.int32), ('bin_lo', np.int32), ('bin_hi', np.int32), ('reserved', np.int32),
                      ('lag0', np.float64), ('g_e', np.float64), ('g_n', np.float64), ('g_t', np.float64)])
CELL_DTYPE = np.dtype([('score', np.float32), ('lag', np.int32)])


def tree_sum(x):
    """The kernel's sum of a float32 vector: 256 strided shares, then adjacent pairs."""
    x = np.asarray(x, np.float32)
    pad = (-len(x)) % 256
    x = np.concatenate([x, np.zeros(pad, np.float32)]).reshape(-1, 256)       # (adding +0 changes nothing)
    s = np.zeros(256, np.float32)
    for row in x:
        s = s + row
    while len(s) > 1:
        s = s[0::2] + s[1::2]
    return s[0]


def row_stats(S):
    """(mean, std) of one surface as step a forms them."""
    S = np.asarray(S, np.float32)
    inv = np.float32(1.0) / np.float32(len(S))
    mean = tree_sum(S) * inv
    d = S - mean
    return mean, np.sqrt(tree_sum(d * d) * inv)


def normalise(rows, sat, pool=1):
    """z of one satellite: rows float32 [nsv][nbins][cs]."""
    cs = rows.shape[2]
    z = None
    for b in range(int(sat['bin_lo']), int(sat['bin_hi']) + 1):
        S = rows[int(sat['row']), b].astype(np.float32)
        mean, sd = row_stats(S)
        if not sd > 0:
            continue
        v = (S - mean) / sd
        z = v if z is None else np.maximum(z, v)
    if z is None:
        z = np.zeros(cs, np.float32)
    if pool > 1:
        z = np.max([np.roll(z, -k) for k in range(pool)], axis=0)
    return z.astype(np.float32)


def collective(rows, sats, grid):
    """The cell map CELL_DTYPE [n_t, n_n, n_e] of one call."""
    sats = np.asarray(sats, SAT_DTYPE)
    cs, w = rows.shape[2], int(grid['pool'])
    z = [normalise(rows, s, w) for s in sats]
    E = grid['e0'] + np.arange(grid['n_e'], dtype=np.float64) * grid['d_e']
    N = grid['n0'] + np.arange(grid['n_n'], dtype=np.float64) * grid['d_n']
    T = grid['t0'] + np.arange(grid['n_t'], dtype=np.float64) * grid['d_t']
    c = np.arange(0, cs, w, dtype=np.float64)
    out = np.zeros((grid['n_t'], grid['n_n'], grid['n_e']), CELL_DTYPE)
    for it in range(grid['n_t']):
        for i_n in range(grid['n_n']):
            score = None
            for p, s in enumerate(sats):
                base = s['lag0'] + s['g_e'] * E + s['g_n'] * N[i_n] + s['g_t'] * T[it]          # [n_e]
                x = base[:, None] + c[None, :]
                i = np.mod(np.floor(x + 0.5), cs).astype(np.int64)
                v = z[p][i]
                score = v if score is None else score + v
            k = np.argmax(score, axis=1)                                      # (the first of equal maxima)
            out['score'][it, i_n] = score[np.arange(len(k)), k]
            out['lag'][it, i_n] = (k * w).astype(np.int32)
    return out


def pyramid(rows, ephs, prns, bins, t_gps, pos, radius_m, time_s, f_offset=0.0, pool=8):
    """The driver on numpy rows: -> dict with ecef, t_gps, lag, score, margin, map, model."""
    from gpsmi import snapshot as S
    cs = rows.shape[2]
    pos, t = np.array(pos, np.float64), float(t_gps)
    model = S.collective_model(ephs, prns, t, pos, cs, f_offset)
    res = {'levels': []}
    for k, level in enumerate(S.collective_levels(radius_m, time_s, cs, float(np.abs(model['g_t']).max()), pool)):
        sats, grid = S.collective_level_args(model, bins, level)
        cells = collective(rows, sats, grid)
        # of the cells with the largest score the one nearest to their centroid
        top = np.argwhere(cells['score'] == cells['score'].max())
        it, i_n, ie = top[np.argmin(((top - top.mean(axis=0)) ** 2).sum(axis=1))]
        E, N, T = grid['e0'] + ie * grid['d_e'], grid['n0'] + i_n * grid['d_n'], grid['t0'] + it * grid['d_t']
        if k == 0:
            sc = cells['score'].astype(np.float64).ravel()
            res['margin'] = (sc.max() - np.median(sc)) / (1.4826 * np.median(np.abs(sc - np.median(sc))))
        lag_p = sats['lag0'] + sats['g_e'] * E + sats['g_n'] * N + sats['g_t'] * T + cells['lag'][it, i_n, ie] \
            + 0.5 * (level[0] - 1)
        res['levels'].append({'pool': level[0], 'best': (int(it), int(i_n), int(ie)), 'grid': grid,
                              'centre': (pos.copy(), t)})
        east, north, _ = S.enu_axes(pos)
        pos, t = pos + E * east + N * north, t + T
        model = S.collective_model(ephs, prns, t, pos, cs, f_offset)
        clock = lag_p - model['lag0']
        clock = clock[0] + np.mod(clock - clock[0] + cs / 2.0, cs) - cs / 2.0
        res.update(map=cells, grid=grid, score=float(cells['score'][it, i_n, ie]), best=(int(it), int(i_n), int(ie)))
    res.update(ecef=pos, t_gps=t, model=model, lag=float(np.mod(np.median(clock), cs)))
    return res


# ---- the weak scene: snapshot_truth's strong geometry (eight satellites, 1 s), every satellite at
# one C/N0.  C/N0 = amp^2 fs / sigma^2 with sigma 0.35 and fs 2.048 Msps.
SCENE_SECONDS = 1.0
SCENE_OFF_M, SCENE_OFF_S = 10.0e3, 1.0              # the a-priori: 10 km and 1 s off the truth
SCENE_RADIUS_M, SCENE_TIME_S = 15.0e3, 2.0


def scene_amp(cn0_dbhz, fs=2048000.0, sigma=0.35):
    return sigma * np.sqrt(10.0 ** (cn0_dbhz / 10.0) / fs)


def weak_scene(cn0_dbhz):
    """(scene, info, complex64 samples) of the strong scene's geometry with all satellites at cn0_dbhz."""
    import snapshot_truth as T
    from gpsmi import synth_nav
    from gpsmi.synth import raw_to_c64
    sc, info = synth_nav.geometric_scene(T.TRUTH, SCENE_SECONDS, n_sats=8, seed=79)
    for s in sc.sats:
        s.amp = float(scene_amp(cn0_dbhz))
    n = int(round(SCENE_SECONDS * 1000)) * sc.code_samples
    return sc, info, raw_to_c64(sc.block_raw(0, n=n))


def scene_apriori(info):
    """The a-priori of the scene: SCENE_OFF_M from the truth (6 km east, 8 km north), the time
    SCENE_OFF_S late."""
    from gpsmi import snapshot as S
    east, north, _ = S.enu_axes(info['truth'])
    return info['truth'] + 0.6 * SCENE_OFF_M * east + 0.8 * SCENE_OFF_M * north, info['t0_gps'] + SCENE_OFF_S


def deep_rows(data, freqs, prns, n_coh, n_seg, p, carrier_hz=1575.42e6, f_offset=0.0):
    """deep_ref.deep_table's surfaces themselves, float32 [nsv][nbins][cs]: the same oracle calls, sum
    order and scale."""
    import gps_oracle as orc
    from deep_ref import deep_shifts
    cs = p.code_samples
    t = orc.sec_time(p)
    spectra = {s: orc.fft_cacode(s, cs) for s in prns}
    span = n_coh * cs
    scale = np.float32(1.0 / n_seg)
    m = deep_shifts(freqs, n_coh, n_seg, cs, carrier_hz, f_offset)
    out = np.zeros((len(prns), len(freqs), cs), np.float32)
    for b, f in enumerate(freqs):
        acc = [np.zeros(cs, np.float32) for _ in prns]
        for g in range(n_seg):
            wiped, _ = orc.demod_doppler(data[g * span:(g + 1) * span], f, 0, span, t)
            spec = orc.folded_spectrum(wiped, 0, n_coh, cs)
            for j, s in enumerate(prns):
                corr = orc.circ_corr(spec, spectra[s])
                if m[b, g] % cs:
                    corr = np.roll(corr, -int(m[b, g]))
                acc[j] = acc[j] + corr
        for j in range(len(prns)):
            out[j, b] = acc[j] * scale
    return out


def scene_search(data, info, cfg, n_coh=4):
    """What collective_search does ahead of its pyramid, on the restated search: the PRNs, bins and
    surfaces at the scene's a-priori.  Only the cells a satellite's window names are computed (the
    others stay zero: the kernels compute them, nothing reads them).  -> (prns, freqs, bins, rows)."""
    import gps_oracle as orc
    from gpsmi import snapshot as S
    pos, t = scene_apriori(info)
    prns, freqs, bins = S.collective_plan_bins(info['ephs'], t, pos, cfg)
    cs = cfg.code_samples
    n_seg = len(data) // cs // n_coh
    rows = np.zeros((len(prns), len(freqs), cs), np.float32)
    for (r, lo, hi), prn in zip(bins, prns):
        rows[r, lo:hi + 1] = deep_rows(data[:n_seg * n_coh * cs], freqs[lo:hi + 1], [prn], n_coh, n_seg,
                                       orc.Params())[0]
    return prns, freqs, bins, rows


def passing(rows, bins, corr_min=8.0):
    """The satellites measure()'s threshold passes, restated on the satellites' own windows: the
    largest peak among the bins with normMaxCorr = (peak - mean) / std > corr_min (float64, as
    acquisition.norm_max_corr).  -> indices."""
    out = []
    for r, lo, hi in bins:
        S_ = rows[r, lo:hi + 1].astype(np.float64)
        nmc = (S_.max(axis=1) - S_.mean(axis=1)) / S_.std(axis=1)
        if (nmc > corr_min).any():
            out.append(r)
    return out
