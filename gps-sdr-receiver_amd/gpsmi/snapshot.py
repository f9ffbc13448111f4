"""Snapshot fix: a position from a fraction of a second of signal, stored ephemerides and a rough
idea of time and place -- no decoded subframe.

``measure`` runs the stages the weak path already has on one uploaded snapshot (deep search ->
refinement -> optionally bit-synchronous tracking, all on the GPU) and returns per satellite a
code phase that is ambiguous by one code period, a Doppler and C/N0.  ``coarse_time_fix`` is the
navigation step that works without decoded time: Gauss-Newton over ECEF position, a
sub-millisecond clock bias and the coarse time, with the whole milliseconds of every satellite
derived from the a-priori position and time relative to the strongest satellite.
``doppler_fix`` makes an a-priori position from the Dopplers alone when the caller has none, and
``snapshot_fix`` chains the three.  ``collective_search`` is the way in when every
satellite is under measure's threshold: the deep surfaces of all visible satellites added over a grid
of position, coarse time and clock.  Everything in this module but the engine calls inside
``measure`` and ``collective_search`` is host float64 numpy.

Contract of ``coarse_time_fix``: the a-priori position within 50 km and the time within 30 s, or
the position within 75 km at the right time, or the time within 90 s at the right position (the
a-priori range errors of any two satellites must differ by less than half of c * 1 ms =
149.9 km: 2 |position error| + 1.6 km/s |time error| < 150 km).  No atmosphere model, as in
position.least_squares_pos4; the ephemerides must be the set valid at that time.  Five satellites
leave no redundancy: the fix is then only as good as the a-priori, and is refused when it ends
outside the region around it.  Six leave one degree of freedom: a solution that fails the
residual test is refused; one bad satellite is dropped only from seven on.  Every fix carries
`protect_m`, the position error one bad measurement could cause without failing the test.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from . import position as P

L1_HZ = 1575.42e6
C_MS = P.GPS_C * 1.0e-3                  # metres of one code period
MIN_SAT = 5
FREEZE_AFTER = 3                         # iterations that re-derive the millisecond integers
MAX_IT = 12
STEP_TOL = 1.0e-4                        # metres: the Gauss-Newton step that ends the iteration
RMS_MAX_SAMPLES = 1.0                    # post-fit residual rms a fix may have, in samples
REGION_M, REGION_M_PER_S = 150.0e3, 1.6e3
TRACK_MIN_SECONDS, TRACK_MIN_BITS = 0.5, 4
EDGE_MIN_BITS = 10                       # bits refinement must span for `edge` (no transition in them: 2^-9)
DEFAULT_SOURCE = 'track'                 # where it applies; the comparison is in DESIGN.md 4.2i

# prn; sample: the stream index the code phase refers to; code_phase: samples in [0, cs), a code
# start lies at sample + code_phase modulo cs; f_hz: as of the middle of the data; cn0_dbhz:
# refinement's; edge: the stream position of a bit edge ('track': the code start itself; NaN when
# refinement spanned fewer than EDGE_MIN_BITS bits), recorded and not used yet; source: b'refine' or b'track'
MEAS_DTYPE = np.dtype([('prn', np.int32), ('sample', np.int64), ('code_phase', np.float64),
                       ('f_hz', np.float64), ('cn0_dbhz', np.float64), ('edge', np.float64),
                       ('source', 'S6')])


# ---------------------------------------------------------------- the range model
def modelled_range(eph, t_rx, pos, rounds=3):
    """c * (reception time - satellite clock reading at transmission) of a signal received at GPS
    time `t_rx` at ECEF `pos`: the geometric range with the receiver displaced by the Earth's
    rotation during the flight (position.sagnac_shift) minus c * the satellite clock correction.
    The transmit time is a fixed point: the first round leaves 12 m of range at the most, the
    second 0.2 mm, the third nothing a float64 holds.
    -> (range in m, unit vector from the satellite to the receiver)."""
    pos = np.asarray(pos, dtype=np.float64)
    v = np.array([-pos[1], pos[0], 0.0]) * P.OMEGA_EARTH
    tau, dt_sv = 0.072, 0.0
    for _ in range(rounds):
        x, y, z, dt_sv = P.sat_ecef(1, eph, DT=t_rx - tau + dt_sv)
        d = np.array([x, y, z]) - pos - v * tau
        tau = np.sqrt(d.dot(d)) / P.GPS_C
    rho = tau * P.GPS_C
    return rho - P.GPS_C * dt_sv, -d / rho


def _rates(ephs, prns, t_rx, pos, rate_dt=0.5):
    """Range rates: the central difference of the modelled range over +-rate_dt (two rounds of
    the fixed point: 0.2 mm over a second is far below what a rate is used for here)."""
    return np.array([(modelled_range(ephs[int(prn)], t + rate_dt, pos, 2)[0]
                      - modelled_range(ephs[int(prn)], t - rate_dt, pos, 2)[0]) / (2.0 * rate_dt)
                     for prn, t in zip(prns, t_rx)])


def _model(ephs, prns, t_rx, pos):
    """Modelled ranges, unit vectors and range rates of `prns` at the reception times `t_rx`."""
    n = len(prns)
    f, e = np.empty(n), np.empty((n, 3))
    for i, prn in enumerate(prns):
        f[i], e[i] = modelled_range(ephs[int(prn)], t_rx[i], pos)
    return f, e, _rates(ephs, prns, t_rx, pos)


def cn0_weights(cn0_dbhz):
    """Weights of the code phases: proportional to C/N0 (the variance of a code-phase estimate
    falls with it), the strongest 1; a satellite without a reading counts as the weakest."""
    cn0 = np.asarray(cn0_dbhz, dtype=np.float64)
    if not np.isfinite(cn0).any():
        return np.ones(len(cn0))
    cn0 = np.where(np.isfinite(cn0), cn0, np.nanmin(cn0))
    return 10.0 ** ((cn0 - cn0.max()) / 10.0)


@dataclass
class Fix:
    ok: bool = False
    reason: str = ''
    ecef: object = None                  # ECEF metres, None unless ok
    t_gps: float = None                  # GPS seconds of week of stream index `sample`
    sample: int = 0
    bias_m: float = 0.0                  # the clock bias, within half a code period
    prns: list = field(default_factory=list)        # the satellites of the solution
    residuals: object = None             # metres, per satellite of `prns`
    integers: object = None              # whole milliseconds relative to `ref_prn`
    ref_prn: int = 0
    dropped: list = field(default_factory=list)     # what the residual test took out
    g: float = float('nan')              # sqrt tr of the position block of inv(H' H)
    rms_m: float = float('nan')           # weighted rms of the residuals
    test_m: float = float('nan')          # ... per degree of freedom: rms * sqrt(n / (n - 5)), what is tested
    protect_m: float = float('inf')       # the position error one bad measurement can cause and pass the test
    moved_m: float = float('nan')   # 2 |position change| + 1.6 km/s |time change| from the a-priori
    iterations: int = 0
    tau: object = None                    # tested figure per metre of bias on each satellite
    slope: object = None                  # position error per unit of the tested figure, per satellite
    path: str = 'measure'                 # what supplied the measurements: 'measure' or 'collective' (snapshot_fix)
    spoof: object = field(default=None, compare=False, repr=False)   # snapshot_fix(..., spoof=True): the SpoofReport


def _solve(prns, samples, phases, w, ephs, clock, pos0, fs):
    """Gauss-Newton over (position, bias, coarse time) for one set of satellites.  clock =
    (stream index, a-priori GPS time of it); the solution's time is that of the strongest
    satellite's `sample`."""
    ref = int(np.argmax(w))
    sample = int(samples[ref])
    t0 = clock[1] + (sample - clock[0]) / fs
    d = ((samples - sample) + phases) / fs           # seconds from `sample` to each code start
    # the code phases as fractional pseudoranges: where the millisecond grid lies is the a-priori
    # time's choice, which the bias absorbs (the fraction is taken first: t0 + d would round)
    z = P.GPS_C * np.mod(np.mod(t0, 1.0e-3) + d, 1.0e-3)
    pos, bias, dt = np.array(pos0, dtype=np.float64), 0.0, 0.0
    N = np.zeros(len(prns))
    fix = Fix(sample=sample, prns=[int(p) for p in prns], ref_prn=int(prns[ref]))
    sw = np.sqrt(w)
    for it in range(MAX_IT):
        f, e, fd = _model(ephs, prns, t0 + dt + d, pos)
        r = z - f
        if it < FREEZE_AFTER:
            N = np.rint((r - r[ref]) / C_MS)
            if it == 0:
                bias = r[ref]
        y = r - N * C_MS - bias
        H = np.column_stack([e, np.ones(len(prns)), fd])
        step = np.linalg.lstsq(H * sw[:, None], y * sw, rcond=None)[0]
        pos, bias, dt = pos + step[:3], bias + step[3], dt + step[4]
        fix.iterations = it + 1
        if not np.all(np.isfinite(step)) or np.linalg.norm(pos) > 1.0e8 or abs(dt) > 1.0e5:
            fix.reason = 'diverged'
            return fix
        if it >= FREEZE_AFTER and np.linalg.norm(step[:4]) < STEP_TOL:
            break
    else:
        fix.reason = 'no convergence'
        return fix
    f, e, fd = _model(ephs, prns, t0 + dt + d, pos)
    r = z - f
    y = r - N * C_MS - bias
    H = np.column_stack([e, np.ones(len(prns)), fd])
    cov = np.linalg.pinv(H.T @ H)
    fix.g = float(np.sqrt(np.trace(cov[:3, :3])))
    fix.residuals, fix.integers = y, N.astype(np.int64)
    fix.rms_m = float(np.sqrt(np.sum(w * y * y) / np.sum(w)))
    dof = len(prns) - 5
    fix.test_m = fix.rms_m * np.sqrt(len(prns) / dof) if dof > 0 else 0.0
    # what one bad measurement can do unseen: a bias b on satellite i moves the position by
    # b |A[:3, i]| and the tested figure by b tau_i (A the solution map, S = I - H A the residual map)
    A = np.linalg.pinv(H.T @ (H * w[:, None])) @ (H * w[:, None]).T
    Sm = np.eye(len(prns)) - H @ A
    fix.tau = np.sqrt(np.sum(w[:, None] * Sm * Sm, axis=0) / np.sum(w) * len(prns) / max(dof, 1)) if dof > 0 \
        else np.zeros(len(prns))
    fix.slope = np.linalg.norm(A[:3], axis=0) / np.maximum(fix.tau, 1.0e-12)
    fix.bias_m = float(bias - np.rint(bias / C_MS) * C_MS)
    fix.t_gps = float(t0 + dt)
    fix.ecef = pos
    fix.moved_m = float(2.0 * np.linalg.norm(pos - pos0) + REGION_M_PER_S * abs(dt))
    if np.any(np.rint((r - r[ref]) / C_MS) != N):
        fix.reason = 'the millisecond integers do not hold at the solution'
    return fix


def coarse_time_fix(meas, ephs, t_gps, pos, weights=None, code_samples=2048):
    """Coarse-time navigation: `meas` (records with prn, sample, code_phase in samples and
    cn0_dbhz; MEAS_DTYPE), `ephs` {prn: ephemeris}, `t_gps` the GPS seconds of week of the
    strongest satellite's `sample` as far as known, `pos` the a-priori ECEF position -- within the
    region of the module docstring.  `weights`: per record, default cn0_weights.  -> Fix; a Fix
    that is not ok carries the reason and no position.

    With six satellites or more the post-fit residual rms per degree of freedom (rms * sqrt(n /
    (n - 5))) is tested against RMS_MAX_SAMPLES.  From seven on, a solution above it is solved
    again with each satellite left out in turn, the best of those that pass replaces it (one
    satellite dropped, once), and a solution that stays above is not ok.  Six satellites that fail
    are refused: five of them would fit anything.  With five there is nothing to test, so the fix
    must end inside the region around the a-priori that
    guarantees its integers."""
    meas = np.asarray(meas)
    keep = [i for i, p in enumerate(meas['prn']) if int(p) in ephs]
    meas = meas[keep]
    if len(meas) < MIN_SAT:
        return Fix(reason=f'{len(meas)} satellites with an ephemeris, {MIN_SAT} needed')
    if len(set(meas['prn'].tolist())) < len(meas):
        return Fix(reason='a satellite is measured twice')
    fs = 1000.0 * code_samples
    w = cn0_weights(meas['cn0_dbhz']) if weights is None else np.asarray(weights, np.float64)[keep]
    prns = meas['prn'].astype(np.int64)
    samples, phases = meas['sample'].astype(np.int64), meas['code_phase'].astype(np.float64)
    clock = (int(samples[int(np.argmax(w))]), float(t_gps))
    pos0 = np.asarray(pos, dtype=np.float64)
    rms_max = RMS_MAX_SAMPLES * P.GPS_C / fs

    def good(fx):
        return not fx.reason and fx.test_m <= rms_max

    fix = _solve(prns, samples, phases, w, ephs, clock, pos0, fs)
    # (a set left with five satellites fits anything: one is dropped only from seven or more)
    if len(prns) > MIN_SAT + 1 and not good(fix):
        for k in range(len(prns)):
            m = np.arange(len(prns)) != k
            fx = _solve(prns[m], samples[m], phases[m], w[m], ephs, clock, pos0, fs)
            fx.dropped = [int(prns[k])]
            if good(fx) and (not good(fix) or fx.test_m < fix.test_m):
                fix = fx
    if not fix.reason and len(fix.prns) > MIN_SAT and fix.test_m > rms_max:
        fix.reason = f'residual rms per degree of freedom {fix.test_m:.1f} m above {rms_max:.1f} m'
    if not fix.reason and len(fix.prns) == MIN_SAT and fix.moved_m >= REGION_M:
        fix.reason = 'five satellites and a solution outside the region around the a-priori'
    if fix.residuals is not None:
        fix.protect_m = float(np.max(fix.slope) * rms_max) if len(fix.prns) > MIN_SAT else float('inf')
    fix.ok = not fix.reason
    if not fix.ok:
        fix.ecef = None
    return fix


# ---------------------------------------------------------------- a-priori from the Dopplers
def doppler_fix(meas, ephs, t_gps, f_offset=0.0, max_it=30):
    """Position and a common frequency offset from the Dopplers alone (`meas`: prn, f_hz), at
    least four satellites: f_hz = -L1 / c * (range rate) + offset, Gauss-Newton from the point on
    the Earth's surface under the mean satellite direction.  Kilometres at best (1 Hz is about
    1.3 km): it is the a-priori position for coarse_time_fix when the caller has none, nothing more.
    -> (ecef, clock_drift_hz)."""
    meas = np.asarray(meas)
    meas = meas[[i for i, p in enumerate(meas['prn']) if int(p) in ephs]]
    if len(meas) < 4:
        raise ValueError(f'{len(meas)} Dopplers with an ephemeris, 4 needed')
    prns = meas['prn'].astype(np.int64)
    t = np.full(len(prns), float(t_gps))
    obs = (meas['f_hz'] - f_offset) * (-P.GPS_C / L1_HZ)          # range rates, m/s
    up = np.zeros(3)
    for prn in prns:
        x = np.array(P.sat_ecef(1, ephs[int(prn)], DT=float(t_gps))[:3])
        up += x / np.linalg.norm(x)
    pos, drift = 6371.0e3 * up / np.linalg.norm(up), 0.0
    h = 1.0e3
    for _ in range(max_it):
        fd = _rates(ephs, prns, t, pos)
        J = np.ones((len(prns), 4))
        for a in range(3):
            dp = np.zeros(3)
            dp[a] = h
            J[:, a] = (_rates(ephs, prns, t, pos + dp) - _rates(ephs, prns, t, pos - dp)) / (2 * h)
        step = np.linalg.lstsq(J, obs - fd - drift, rcond=None)[0]
        n = np.linalg.norm(step[:3])
        if n > 1.0e6:                                # (a long way off the model is not linear)
            step *= 1.0e6 / n
        pos, drift = pos + step[:3], drift + step[3]
        if n < 10.0:                                 # (1 Hz of Doppler noise is a kilometre)
            break
    return pos, float(-drift * L1_HZ / P.GPS_C)


# ---------------------------------------------------------------- measurements on the GPU
def drop_ghosts(rec):
    """DESIGN.md 4.2h's rule (pipeline.ghosts_of) among the records of one refinement call: a
    record that is another one's satellite seen through the wrong code.  -> bool per record,
    True = ghost."""
    from .pipeline import ghosts_of
    out = np.zeros(len(rec), bool)
    for k, o in enumerate(rec):
        hit = ghosts_of(o, rec)
        hit[k] = False
        out |= hit
    return out


def _bit_line(bits, n_bits, pull_in, cs, mid_sample):
    """The straight line through the code starts of the bits behind pull-in against their nominal
    positions, read at the middle one, and the Doppler line read at `mid_sample`.
    -> (tau, f_hz) or None when too few bits are left."""
    b = bits[pull_in:n_bits]
    if len(b) < TRACK_MIN_BITS:
        return None
    x = (b['bit_no'] - b['bit_no'][len(b) // 2]).astype(np.float64)
    nominal = x * 20.0 * cs
    tau_mid = np.polyfit(x, b['tau'] - b['tau'][len(b) // 2] - nominal, 1)[1] + b['tau'][len(b) // 2]
    pf = np.polyfit(b['tau'] - mid_sample, b['f_hz'], 1)
    return float(tau_mid), float(pf[1])


def refined_records(rec, found, cs, f_offset=0.0):
    """The records of refinement (and the hits they were refined from) that count -- confirmed,
    with a code phase, no ghost -- and their MEAS_DTYPE records as of the first sample.
    -> (rec, found, records)."""
    good = (rec['confirmed'] == 1) & (rec['code_phase'] >= 0) & ~drop_ghosts(rec)
    rec, found = rec[good], [h for h, g in zip(found, good) if g]
    out = np.zeros(len(rec), MEAS_DTYPE)
    tap = 1 if cs == 2048 else 8
    Tc = cs / (1.0 + (rec['f_hz'] - f_offset) / L1_HZ)
    out['prn'], out['f_hz'], out['cn0_dbhz'] = rec['prn'], rec['f_hz'], rec['cn0_dbhz']
    out['code_phase'] = np.mod(rec['code_phase'], cs)
    # (refinement counts edge_ms from one period later when the delay is below the tap spacing)
    late = np.array([1.0 if h[3] < tap else 0.0 for h in found])
    out['edge'] = rec['code_phase'] + (rec['edge_ms'] + late) * Tc
    # (without a transition in the data no edge shows: fewer than EDGE_MIN_BITS bits leave a chance)
    out['edge'][rec['n_bits'] < EDGE_MIN_BITS] = np.nan
    out['source'] = b'refine'
    return rec, found, out


def tracked_records(out, bits, n_done, n, cs, pull_in_bits=0):
    """Replaces, in place, the records of refined_records by what the tracked bits say: bits
    [nhits, n_bits] and n_done (bits each channel got through) of trackHits on the `n` samples."""
    pull_in = 10 if pull_in_bits == 0 else max(int(pull_in_bits), 0)         # (track_weak's default)
    for i in range(len(out)):
        line = _bit_line(bits[i], int(n_done[i]), pull_in, cs, 0.5 * n)
        if line is not None:
            tau, f = line
            k = int(np.floor(tau))
            out[i] = (out['prn'][i], k, tau - k, f, out['cn0_dbhz'][i], tau, b'track')


def min_samples(cs):
    """The shortest snapshot: what Acquisition.refineHits needs for n_ms = 40 (two code periods and
    the tap spacing in hand for the code slide), 86017 samples at 2048."""
    return 42 * cs + (1 if cs == 2048 else 8)


CANCEL_DBHZ = 40.0                       # measure(cancel=True): what counts as a strong satellite


def _measure_pass(acq, dev, n, prns, freqs, n_coh, n_seg, corr_min, f_offset, st):
    """Deep search, refinement and the records that count, on device-resident data.
    -> (rec, found, records), all empty when nothing is found."""
    from .pipeline import largest_peak_hits, refine_centred
    cs = acq.cfg.code_samples
    found = largest_peak_hits(acq, (dev[0], n_seg * n_coh * cs), prns, freqs, n_coh, n_seg, f_offset=f_offset,
                              corr_min=corr_min)
    st['device_ms'] += acq.engine.last_ms()
    if not found:
        return None, [], np.zeros(0, MEAS_DTYPE)
    found, rec, ms = refine_centred(acq, dev, found, f_offset=f_offset)
    st['device_ms'] += ms
    st['found'], st['refined'] = st['found'] + found, rec if st['refined'] is None else np.concatenate([st['refined'], rec])
    return refined_records(rec, found, cs, f_offset)


# ---------------------------------------------------------------- the spoofing check
SPOOF_REL_DB = 12.0                      # a PRN's second record must read within this of its strongest
SPOOF_MIN_DOUBLED = 2                    # doubled PRNs that raise the alarm
SPOOF_MAX_DOUBLED = 8                    # doubled PRNs the twin fixes enumerate: 2^7 assignments
SPOOF_PICKS = 4                          # peaks taken per PRN
SPOOF_REFINE_HITS = 64                   # hits of one refinement call (kRefMaxHits)
# the least |v_i^H v_j| at which two records count as one source.  Measured on the
# four-antenna spoofed scene of tests/sig_ref.py: the restated chain over 64 ms
# (tests/test_snapshot_signature.py) puts the least same-source pair at 0.9985 and the pairs of the
# authentic set at 0.0093 .. 0.688; the GPU path over the whole second (MI355X,
# tests/test_gpu_snapshot_signature.py) at 0.9999 and a least authentic pair of 0.0012.  0.95 leaves
# more than thirty times the larger same-source deviation from 1
SPOOF_RHO_MIN = 0.95
SPOOF_DIRECTION_PRNS = 4                 # distinct PRNs from one direction that raise the alarm by themselves


@dataclass
class SpoofReport:
    """What measure(..., spoof=True) and snapshot_fix(..., spoof=True) say about a snapshot.  It
    names PRNs that are in the air twice and, where both sets solve, two positions; with one antenna
    it makes no claim about which of them is authentic.  With `antennas` every
    record has a spatial signature, and the set whose doubled records all arrive from one direction
    is the spoofer's: `authentic` names the other fix."""
    doubled: list = field(default_factory=list)     # PRNs with two records
    alarm: bool = False                             # len(doubled) >= min_doubled
    crowded: bool = False                           # a PRN had more than two records that count: the two strongest stayed
    prns: list = field(default_factory=list)        # the PRN of every row of `picks`
    picks: object = None                            # PEAKS_PICK_DTYPE [len(prns)][k] (None off the GPU path)
    fixes: tuple = None                             # snapshot_fix: (fix_a, fix_b), or (the single fix, None)
    separation_m: float = None                      # |fix_a - fix_b|, None without two fixes
    assignments: int = 0                            # pairs of sets that were solved
    sets: tuple = None                              # the record indices behind `fixes` (None without two fixes)
    antennas: int = 0                               # the coherent channels the signatures were taken over (0: none)
    signature: object = None                        # complex128 [records][antennas]: signature_vectors, per record
    quality: object = None                          # float64 [records]: largest eigenvalue over the mean of the others
    rho: object = None                              # float64 [records][records]: signature_rho
    one_source: tuple = (False, False)              # per set of `sets`: its doubled records arrive from one direction
    one_direction: bool = False                     # SPOOF_DIRECTION_PRNS or more PRNs, every record from one direction
    authentic: object = None                        # 0 or 1 into `fixes`; None without a verdict
    profile_t: object = None                        # float64 [records]: ProfileFit.T per record (None without profile=True)
    distorted: list = field(default_factory=list)   # PRNs with a record whose profile needs a second path
    profile: list = None                            # ProfileFit per record


def spoof_keep(rec, found, cs, f_offset=0.0, min_doubled=SPOOF_MIN_DOUBLED):
    """The keep rule of the spoofing check on the refinement records `rec` of the hits `found`
    (several per PRN): refined_records' rule (confirmed, a code phase, no ghost), then per PRN the
    records reading within SPOOF_REL_DB of its strongest by refinement's C/N0 -- the code's
    autocorrelation sidelobes lie 24 dB down, a spoofer that means to capture a loop within a few
    dB -- and of those the two strongest.  -> (rec, found, MEAS_DTYPE records sorted by PRN, a PRN
    may appear twice; SpoofReport with doubled, alarm and crowded)."""
    rec, found, out = refined_records(rec, found, cs, f_offset)
    cn0 = np.where(np.isfinite(rec['cn0_dbhz']), rec['cn0_dbhz'], -np.inf).astype(np.float64)
    keep, report = [], SpoofReport()
    for prn in sorted(set(rec['prn'].tolist())):
        idx = np.flatnonzero(rec['prn'] == prn)
        idx = idx[np.argsort(-cn0[idx], kind='stable')]               # the strongest first
        near = [i for i in idx if cn0[i] >= cn0[idx[0]] - SPOOF_REL_DB]
        report.crowded = report.crowded or len(near) > 2
        keep += sorted(near[:2])
        if len(near) >= 2:
            report.doubled.append(int(prn))
    report.alarm = len(report.doubled) >= min_doubled
    keep = np.array(keep, dtype=np.int64)
    return rec[keep], [found[i] for i in keep], out[keep], report


# ---------------------------------------------------------------- correlation profiles
# the least T (ProfileFit) at which a record's profile counts as distorted.  Measured on the CPU through
# the restated chain (tests/test_profile.py: test_snapshot_spoof.py's chain, then tests/profile_ref.py on
# its records): the eight records of the clean strong scene read T = 1.88 .. 5.59 (the strong satellites'
# cross-correlations and what the one-path model leaves of the sub-sample sweep; white noise alone gives
# about 1), the sixteen of the 30-us spoofed scene 1.42 .. 3.86 (the copies lie 52 .. 67 lags away, outside
# the taps).  Twice the largest: 2 x 5.59.  The lift-off scene (tests/liftoff_truth.py: copies 0.16 .. 1.94
# samples behind the authentic codes, +3 dB) reads 325.6, 80.2 and 76.9 on the three PRNs whose copies lie
# 1.8 samples or more away -- 29, 7.2 and 6.9 times the threshold -- 14.4 at 1.40 samples, and 4.1 .. 9.5
# on the four whose copies lie within a sample (not flagged: within half a chip the sweep of a single path
# and a second path look alike to whole-sample windows).  The MI355X path reads the same T to 8.1e-7
# relative (tests/test_gpu_snapshot_profile.py)
PROFILE_T_MIN = 11.2
# the least snr1 at which a record's T counts: E1 over the noise of one run and dimension.  A record of
# 33 dB-Hz summed over a 20-ms run reads 10^((33 - 17) / 10) = 40; below that the two delays are fitted to
# noise as much as to the signal and the record is left to the peaks' check
PROFILE_SNR1_MIN = 40.0
PROFILE_STEP = 1.0 / 16.0                # the template grid at 2048: samples
PROFILE_SPAN = 3.0                       # ... over +- this many samples
PROFILE_ORTH_MIN = 1.0e-6                # a second delay's part orthogonal to the first, of its norm
PROFILE_SMEAR = 0.5                      # samples a single path's delay may lie off the best one: whole-sample windows
PROFILE_RANK = 3                         # directions of the one-path model: the template, its slope, its curvature


@dataclass
class ProfileFit:
    """profile_fit's result for one record.  T: the energy a second code replica picks up beyond the
    best single one, over the noise per run and dimension (about 1 when one replica explains the
    profile); snr1: the same for the best single replica.  d1, d2: the delays of the two replicas in
    samples behind the window start (the record's own code start lies `frac` behind it); rel_power:
    the second path's power over the first's in the two-column least squares."""
    prn: int = 0
    n_runs: int = 0
    T: float = np.nan
    snr1: float = np.nan
    e1: float = np.nan
    e2x: float = np.nan
    sigma2: float = np.nan
    d1: float = np.nan
    d2: float = np.nan
    frac: float = 0.0
    rel_power: float = np.nan


def _replica_f32(prn, cs):
    from . import codes
    return codes.code_replica(int(prn), cs).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=64)
def profile_noise(prn, cs, half_taps):
    """N[l][l'] = r(l - l') / cs, r the autocorrelation of the sampled replica (the colour the taps of
    white noise have), float64 [K][K], read-only."""
    R = _replica_f32(prn, cs)
    K = 2 * half_taps + 1
    r = np.array([R[k:] @ R[:cs - k] for k in range(K)]) / cs
    idx = np.abs(np.arange(K)[:, None] - np.arange(K)[None, :])
    out = r[idx]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def profile_template(prn, cs, half_taps):
    """The analytic template: g_d[l] = sum_i c(l + i - d) R[i], the continuous code c starting d
    samples behind the window start against the sampled replica R.  c is the function R samples:
    GPSCacode's own interpolant -- the chips doubled to 2046 knots, joined by straight lines, one
    period over cs samples -- so that g_0 is the replica's own autocorrelation.  The grid is
    d = -PROFILE_SPAN .. +PROFILE_SPAN in steps of PROFILE_STEP samples at 2048, both scaled by
    cs / 2048 so that they cover the same chips at another rate.
    -> (d float64 [nd], g float64 [nd][K]), read-only."""
    from . import codes
    R = _replica_f32(prn, cs)
    y = np.repeat(codes.ca_chips(int(prn)).astype(np.float64), 2)     # 2046 knots, periodic
    y = np.append(y, y[0])
    knots_per_sample = (len(y) - 2.0) / (cs - 1.0)
    scale = cs / 2048.0
    nd_half = int(round(PROFILE_SPAN / PROFILE_STEP))
    d = np.arange(-nd_half, nd_half + 1) * (PROFILE_STEP * scale)
    K = 2 * half_taps + 1
    u = np.arange(-half_taps, cs + half_taps, dtype=np.float64)
    g = np.empty((len(d), K))
    for q, dq in enumerate(d):
        xk = np.mod((u - dq) * knots_per_sample, len(y) - 1.0)
        j = np.minimum(np.floor(xk).astype(np.int64), len(y) - 2)
        c = (y[j + 1] - y[j]) * (xk - j) + y[j]
        g[q] = np.lib.stride_tricks.sliding_window_view(c, cs) @ R
    d.setflags(write=False), g.setflags(write=False)
    return d, g


def profile_fit(cov, n_runs, prn, frac, cs, half_taps, template=None, smear=None):
    """Does one code replica explain the profile covariance `cov` (complex [K][K] of one record of
    AcqEngine.profiles over `n_runs` runs), or are two needed?  float64 numpy, DESIGN.md 4.2r:
    Q is whitened by the Cholesky factor of profile_noise.  The best single template g_d over the
    grid of delays gives d1.  One path: the windows start on whole samples, so under code Doppler a
    single path's delay behind them sweeps +- half a sample within the second; the one-path model is
    therefore the PROFILE_RANK leading directions of the templates within `smear` samples (default
    PROFILE_SMEAR) of d1, and E1 the energy of Q in them (smear = 0: the one template, rank one).
    Two paths: E2x, the largest energy the part of any g_d' orthogonal to that subspace picks up (a
    d' whose orthogonal part is below PROFILE_ORTH_MIN of its norm is skipped).
    sigma^2 = (tr Q - E1 - E2x) / ((K - rank - 1) n_runs); T = E2x / (n_runs sigma^2); snr1 =
    E1 / (n_runs sigma^2).  `frac`: the record's code start behind its window start at sample 0
    (tau - rint(tau)), carried into the result.  `template`: (d [nd], g [nd][K]) in place of
    profile_template's -- the hook for a front end whose filter rounds the correlation peak.
    -> ProfileFit."""
    K = 2 * int(half_taps) + 1
    Q = np.asarray(cov, dtype=np.complex128)
    if Q.shape != (K, K):
        raise ValueError(f'cov must be [{K}][{K}]')
    d, g = profile_template(int(prn), int(cs), int(half_taps)) if template is None else template
    d, g = np.asarray(d, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if g.shape != (len(d), K):
        raise ValueError(f'template must be (d [nd], g [nd][{K}])')
    smear = PROFILE_SMEAR if smear is None else float(smear)
    Lc = np.linalg.cholesky(profile_noise(int(prn), int(cs), int(half_taps)))
    Qw = np.linalg.solve(Lc, np.linalg.solve(Lc, Q).conj().T).conj().T          # L^-1 Q L^-H
    Qw = 0.5 * (Qw + Qw.conj().T)
    gw = np.linalg.solve(Lc, g.T).T                                              # [nd][K], real
    nrm2 = np.einsum('dk,dk->d', gw, gw)
    e = np.einsum('dk,kj,dj->d', gw, Qw, gw).real / nrm2
    i1 = int(np.argmax(e))
    near = gw[np.abs(d - d[i1]) <= smear + 1e-9]
    rank = min(PROFILE_RANK, len(near)) if smear > 0 else 1
    U = gw[i1][:, None] / np.sqrt(nrm2[i1]) if rank == 1 else np.linalg.svd(near.T, full_matrices=False)[0][:, :rank]
    E1 = float(np.einsum('ka,kj,ja->', U, Qw, U).real)
    orth = gw - (gw @ U) @ U.T
    on2 = np.einsum('dk,dk->d', orth, orth)
    ok = (on2 > PROFILE_ORTH_MIN ** 2 * nrm2) & (np.abs(d - d[i1]) > smear)      # (never d1 itself)
    ok[i1] = False
    e2 = np.full(len(d), -np.inf)
    e2[ok] = np.einsum('dk,kj,dj->d', orth[ok], Qw, orth[ok]).real / on2[ok]
    i2 = int(np.argmax(e2))
    E2x = float(max(e2[i2], 0.0))
    n_runs = int(n_runs)
    sigma2 = (float(np.trace(Qw).real) - E1 - E2x) / ((K - rank - 1) * n_runs)
    G = np.stack([gw[i1], gw[i2]], axis=1)                                       # two-column least squares
    B = np.linalg.solve(G.T @ G, G.T)
    P = np.einsum('ak,kj,aj->a', B, Qw, B).real
    return ProfileFit(prn=int(prn), n_runs=n_runs, T=E2x / (n_runs * sigma2), snr1=E1 / (n_runs * sigma2), e1=E1,
                      e2x=E2x, sigma2=sigma2, d1=float(d[i1]), d2=float(d[i2]), frac=float(frac),
                      rel_power=float(P[1] / P[0]))


def profile_verdict(report, meas, cov, n_runs, cs, half_taps, min_doubled=SPOOF_MIN_DOUBLED, template=None):
    """profile_fit on every record of `meas` (cov [R][K][K], n_runs [R] of AcqEngine.profiles) into
    report.profile and profile_t; report.distorted: the PRNs with a record whose T > PROFILE_T_MIN at an
    snr1 of PROFILE_SNR1_MIN or more; the alarm is raised when the PRNs doubled or distorted count
    `min_doubled`, and an alarm that stands already (doubled PRNs, one_direction) is never taken back."""
    fits = []
    for r in range(len(meas)):
        tau = float(meas['sample'][r]) + float(meas['code_phase'][r])
        fits.append(profile_fit(cov[r], n_runs[r], meas['prn'][r], tau - np.rint(tau), cs, half_taps, template))
    report.profile = fits
    report.profile_t = np.array([f.T for f in fits], dtype=np.float64)
    report.distorted = sorted({f.prn for f in fits if f.T > PROFILE_T_MIN and f.snr1 >= PROFILE_SNR1_MIN})
    # (on top of what is raised already: spoof_resolve's one_direction alarm stands)
    report.alarm = report.alarm or len(set(report.doubled) | set(report.distorted)) >= min_doubled
    return report


def signature_vectors(cov):
    """The signatures of AcqEngine.signatures' covariances complex128 [R][A][A]: per record the
    unit principal eigenvector (numpy.linalg.eigh), turned so that its antenna-0 entry is real and
    not negative, and the largest eigenvalue over the mean of the others (inf when those vanish).
    -> (v complex128 [R][A], quality float64 [R])."""
    cov = np.asarray(cov, dtype=np.complex128)
    v = np.zeros(cov.shape[:2], np.complex128)
    quality = np.zeros(len(cov), np.float64)
    for r, c in enumerate(cov):
        w, vec = np.linalg.eigh(c)
        x = vec[:, -1]
        if abs(x[0]) > 0.0:
            x = x * (np.conj(x[0]) / abs(x[0]))
        x = x / np.linalg.norm(x)
        v[r] = x
        v[r, 0] = abs(x[0])
        rest = float(np.mean(w[:-1]))
        quality[r] = w[-1] / rest if rest > 0.0 else np.inf
    return v, quality


def signature_rho(v):
    """|v_i^H v_j| of unit signatures [R][A] -> float64 [R][R]."""
    v = np.asarray(v, dtype=np.complex128)
    return np.abs(v.conj() @ v.T)


def _least_rho(rho, idx):
    idx = list(idx)
    return min((rho[i, j] for k, i in enumerate(idx) for j in idx[k + 1:]), default=np.inf)


def spoof_resolve(report, meas, sets, v, rho_min=SPOOF_RHO_MIN):
    """The decision on top of the signatures `v` (signature_vectors, one per record of `meas`).
    `sets`: the pair of record-index sets behind report.fixes (None: no pair of fixes).  In each
    set the records of the doubled PRNs count (single records are in both sets); a set is one
    source when it holds at least two of them and their least pairwise rho is >= rho_min.  Exactly
    one such set is the spoofer's and the other fix is authentic; both or neither: no verdict.
    Independently one_direction: the records of SPOOF_DIRECTION_PRNS or more distinct PRNs (twins
    included), all with a least pairwise rho >= rho_min -- a spoofer that has swamped the sky; it
    raises the alarm without a doubled PRN.  Fills report.signature, rho, one_source,
    one_direction, authentic (and alarm).  -> authentic."""
    v = np.asarray(v, dtype=np.complex128)
    rho = signature_rho(v)
    doubled = set(report.doubled)
    prns = [int(p) for p in meas['prn']]
    one = [False, False]
    if sets is not None:
        for s, ix in enumerate(sets):
            twins = [i for i in ix if prns[i] in doubled]
            one[s] = len(twins) >= 2 and bool(_least_rho(rho, twins) >= rho_min)
    report.signature, report.rho, report.one_source = v, rho, (one[0], one[1])
    report.authentic = None if one[0] == one[1] else 1 if one[0] else 0
    report.one_direction = len(set(prns)) >= SPOOF_DIRECTION_PRNS and bool(_least_rho(rho, range(len(prns))) >= rho_min)
    report.alarm = report.alarm or report.one_direction
    return report.authentic


# ---------------------------------------------------------------- per-satellite beams
# a record outside the spoofer's set carries the null when its signature's rho to the null vector is
# at most this: the null costs 1 / (1 - rho^2) of noise gain, exactly 3 dB here
BEAM_NULL_RHO_MAX = float(np.sqrt(0.5))
BEAM_MAX = 64                            # beams of one gpsmi_nul_beams call


def one_source(rho, prns, rho_min=SPOOF_RHO_MIN):
    """What one transmitter sends: the largest set of records (indices into `prns`, ascending) of
    SPOOF_DIRECTION_PRNS or more distinct PRNs whose pairwise rho is all >= rho_min.  A transmitter
    sends a PRN once, so a set holds no PRN twice: of a spoofer's copy and the authentic satellite
    that happens to stand in its direction only one belongs to it.  Of several sets of the largest
    size the tightest, the one whose least pairwise rho is the greatest (then the smallest
    indices).  None without one."""
    rho = np.asarray(rho, dtype=np.float64)
    prns = [int(p) for p in prns]
    n = len(prns)
    adj = [{j for j in range(n) if j != i and prns[j] != prns[i] and rho[i, j] >= rho_min} for i in range(n)]
    best, best_key = None, None

    def grow(clique, cand, done):                   # Bron-Kerbosch with a pivot: every maximal set
        nonlocal best, best_key
        if not cand and not done:
            if len(clique) >= SPOOF_DIRECTION_PRNS:
                ix = sorted(clique)
                key = (-len(ix), -_least_rho(rho, ix), ix)
                if best_key is None or key < best_key:
                    best, best_key = ix, key
            return
        if best is not None and len(clique) + len(cand) < len(best):
            return
        pivot = max(cand | done, key=lambda u: (len(adj[u] & cand), -u))
        for u in sorted(cand - adj[pivot]):
            grow(clique + [u], cand & adj[u], done & adj[u])
            cand, done = cand - {u}, done | {u}

    grow([], set(range(n)), set())
    return best


def beam_plan(meas, cov, v, rho):
    """What measure(..., beams=True) asks of NullSteer.beams for the records `meas`: cov
    (AcqEngine.signatures' covariances [R][A][A]), v (signature_vectors) and rho (signature_rho).
    Every record gets a beam at its own signature.  When one_source finds a set, its null vector is
    the signature of the sum of that set's covariances, each over its trace; a record outside the
    set carries the null iff its rho to that vector is <= BEAM_NULL_RHO_MAX, the set's own records
    carry none.  -> (steer complex128 [R][A], nulls complex128 [1][A] or None, mask uint32 [R],
    info: set (or None), null, rho_null float64 [R])."""
    v = np.asarray(v, dtype=np.complex128)
    cov = np.asarray(cov, dtype=np.complex128)
    mask = np.zeros(len(v), dtype=np.uint32)
    info = {'set': one_source(rho, meas['prn']), 'null': None, 'rho_null': np.zeros(len(v))}
    if info['set'] is None:
        return v.copy(), None, mask, info
    pooled = sum(cov[i] / np.trace(cov[i]).real for i in info['set'])
    u = signature_vectors(pooled[None])[0][0]
    info['null'], info['rho_null'] = u, np.abs(v.conj() @ u)
    outside = np.ones(len(v), dtype=bool)
    outside[info['set']] = False
    mask[outside & (info['rho_null'] <= BEAM_NULL_RHO_MAX)] = 1
    return v.copy(), u[None].copy(), mask, info


def _beam_pass(acq, dev, n, found, out, cov, v, rho, antennas, source, freqs, f_offset, track_cfg, st):
    """measure's beams: one NullSteer of cfg.ngps forms the beams of all records over the whole blocks
    of the snapshot into a complex64 device buffer, and every record is refined again (and, with
    source 'track', tracked) on its own row from its own hit.  Replaces the confirmed records of
    `out` in place; fills st['beams_ms'], st['before_beams'] and st['beams']."""
    from .engine import DeviceBuffer
    from .nulling import NullSteer
    from .pipeline import refine_centred
    c = acq.cfg
    cs = c.code_samples
    st['before_beams'], st['beams'], st['beams_ms'] = out.copy(), [], 0.0
    nb = n // c.ngps
    nn = nb * c.ngps
    if not len(out) or nn < min_samples(cs):
        return
    steer, nulls, mask, info = beam_plan(out, cov, v, rho)
    st['beam_plan'] = info
    step = abs(freqs[1] - freqs[0]) if len(freqs) > 1 else c.step_freq
    was_raw = acq.engine.raw_u8
    ns = NullSteer(c, antennas=antennas, raw_u8=was_raw)
    rows = DeviceBuffer(min(len(out), BEAM_MAX) * nn * 8, c.device)
    try:                                            # the beams are complex64 whatever the data is
        if was_raw:
            acq.engine.set_input_format(False)
        for k0 in range(0, len(out), BEAM_MAX):
            sel = slice(k0, min(k0 + BEAM_MAX, len(out)))
            ns.beams_dev(dev[0], rows.ptr, nb, steer[sel], nulls, mask[sel], in_stride=n, out_stride=nn)
            st['beams_ms'] += ns.last_ms()
            st['device_ms'] += ns.last_ms()
            st['beam_kernel_ms'] = ns.last_beam_kernel_ms()
            flags, gain, w = ns.last_beam_flags, ns.last_beam_gain_db, ns.last_beam_weights
            for j, r in enumerate(range(sel.start, sel.stop)):
                row = (rows.at(j * nn * 8), nn)
                f1, rec1, ms = refine_centred(acq, row, [found[r]], f_offset=f_offset, df_half=float(step))
                st['device_ms'] += ms
                rec1, _, out1 = refined_records(rec1, f1, cs, f_offset)
                entry = {'prn': int(out['prn'][r]), 'null': bool(mask[r]), 'confirmed': len(out1) == 1,
                         'gain_db': float(np.mean(gain[:, j])), 'flags': sorted(set(flags[:, j].tolist())),
                         'weights': w[:, j].copy()}
                st['beams'].append(entry)
                if len(out1) != 1:                  # not confirmed on its beam: the antenna-0 values stay
                    continue
                if source == 'track':
                    _track_records(acq, row, rec1, out1, nn, f_offset, track_cfg, st)
                out[r] = out1[0]
    finally:
        if was_raw:
            acq.engine.set_input_format(True)
        rows.free()
        ns.close()


def _array_pass(acq, dev, n, prns, freqs, n_coh, n_seg, corr_min, antennas, source, f_offset, track_cfg, st):
    """measure's array=True: the array search over all rows, per PRN the largest peak
    over `corr_min` (pipeline.array_peak_hits); the hits' signatures at tau = the argmax and f = the
    bin (AcqEngine.signatures); one beam per hit steered at its signature, no null (NullSteer.beams over
    the whole blocks of the snapshot, complex64); every hit refined on its own beam; the confirmed
    records with a code phase, ghosts dropped over all of them together; with source 'track' each
    tracked on its beam.  A hit whose refinement on the beam is not confirmed is dropped.
    -> records.  Fills st: array_ms, signature_ms, beams_ms, hits, beams, found, refined."""
    from .engine import DeviceBuffer
    from .nulling import NullSteer
    from .pipeline import array_peak_hits, refine_centred
    c = acq.cfg
    cs = c.code_samples
    st.update(array_ms=0.0, signature_ms=0.0, beams_ms=0.0, hits=[], beams=[])
    none = np.zeros(0, MEAS_DTYPE)
    hits = array_peak_hits(acq, dev, antennas, prns, freqs, n_coh, n_seg, f_offset=f_offset, corr_min=corr_min)
    st['array_ms'] = acq.engine.last_ms()
    st['device_ms'] += st['array_ms']
    st['hits'] = list(hits)
    nb = n // c.ngps
    nn = nb * c.ngps
    if not hits or nn < min_samples(cs):
        return none
    cov = acq.engine.signatures(dev, [(s, f, float(d)) for _, s, f, d in hits], antennas, f_offset=f_offset)[0]
    st['signature_ms'] = acq.engine.last_ms()
    st['device_ms'] += st['signature_ms']
    v, quality = signature_vectors(cov)
    st['signature'], st['quality'] = v, quality
    was_raw = acq.engine.raw_u8
    ns = NullSteer(c, antennas=antennas, raw_u8=was_raw)
    rows = DeviceBuffer(len(hits) * nn * 8, c.device)       # (one hit per PRN: 37 rows at the most, <= BEAM_MAX)
    try:                                            # the beams are complex64 whatever the data is
        if was_raw:
            acq.engine.set_input_format(False)
        ns.beams_dev(dev[0], rows.ptr, nb, v, None, np.zeros(len(hits), dtype=np.uint32), in_stride=n, out_stride=nn)
        st['beams_ms'] = ns.last_ms()
        st['device_ms'] += st['beams_ms']
        gain, flags = ns.last_beam_gain_db, ns.last_beam_flags
        row = [(rows.at(j * nn * 8), nn) for j in range(len(hits))]
        found, recs = [], []
        for j, hit in enumerate(hits):
            f1, rec1, ms = refine_centred(acq, row[j], [hit], f_offset=f_offset)
            st['device_ms'] += ms
            found, recs = found + f1, recs + [rec1]
        rec = np.concatenate(recs)
        st['found'], st['refined'] = found, rec
        good = np.flatnonzero((rec['confirmed'] == 1) & (rec['code_phase'] >= 0) & ~drop_ghosts(rec))
        for j, hit in enumerate(hits):
            st['beams'].append({'prn': int(hit[1]), 'confirmed': bool(rec['confirmed'][j] == 1), 'kept': j in good,
                                'gain_db': float(np.mean(gain[:, j])), 'flags': sorted(set(flags[:, j].tolist()))})
        rec, _, out = refined_records(rec, found, cs, f_offset)
        assert len(out) == len(good)
        if source == 'track':
            for k, j in enumerate(good):
                _track_records(acq, row[j], rec[k:k + 1], out[k:k + 1], nn, f_offset, track_cfg, st)
        return out
    finally:
        if was_raw:
            acq.engine.set_input_format(True)
        rows.free()
        ns.close()


def authentic_first(report):
    """With a verdict (spoof_resolve) the authentic fix goes first in report.fixes, whatever order
    twin_fixes gave them; sets and one_source follow and authentic becomes 0.  -> fixes[0]."""
    if report.authentic == 1:
        report.fixes, report.sets = report.fixes[::-1], report.sets[::-1]
        report.one_source, report.authentic = report.one_source[::-1], 0
    return report.fixes[0]


def twin_sets(meas):
    """The complementary assignments of the records of doubled PRNs to two sets: records of
    `meas` (sorted by PRN).  Single records go into both sets; of D doubled PRNs (beyond
    SPOOF_MAX_DOUBLED the ones with the strongest weaker record) the first keeps its order and the
    others take both: 2^(D-1) pairs.  A PRN doubled beyond the limit gives its stronger record to
    both sets.  -> list of (indices of set a, indices of set b)."""
    prns = meas['prn'].tolist()
    pairs = {p: [i for i, q in enumerate(prns) if q == p] for p in sorted(set(prns))}
    doubled = [p for p, ix in pairs.items() if len(ix) == 2]
    weaker = {p: min(meas['cn0_dbhz'][i] for i in pairs[p]) for p in doubled}
    used = sorted(sorted(doubled, key=lambda p: -np.nan_to_num(weaker[p], nan=-np.inf))[:SPOOF_MAX_DOUBLED])
    base = []
    for p, ix in pairs.items():
        if p not in used:
            base.append(ix[0] if len(ix) == 1 else max(ix, key=lambda i: np.nan_to_num(meas['cn0_dbhz'][i], nan=-np.inf)))
    out = []
    for code in range(1 << max(len(used) - 1, 0)):
        a, b = list(base), list(base)
        for j, p in enumerate(used):
            flip = j > 0 and (code >> (j - 1)) & 1
            a.append(pairs[p][1 if flip else 0])
            b.append(pairs[p][0 if flip else 1])
        out.append((sorted(a), sorted(b)))
    return out


def twin_fixes(meas, ephs, t_gps, pos, report, code_samples=2048, have_pos=True):
    """Solves once per consistent assignment (twin_sets) with coarse_time_fix, `t_gps` the GPS time
    of stream index 0 and `pos` the a-priori (the first solution that is ok serves as the a-priori
    of the sets that follow), and takes the pair whose two fixes are both ok with the least sum of
    rms_m.  With an a-priori position of the caller's (`have_pos`) the fix nearer to it goes first,
    otherwise the one with the lower mean C/N0 on its doubled records.  Without such a pair: the
    best single ok fix and None.  Fills report.fixes, separation_m, assignments and sets (per fix the
    indices of the records it is made of: its set without what its residual test dropped).
    -> fix_a (a Fix that is not ok when nothing solved)."""
    fs = 1000.0 * code_samples
    pos0 = np.asarray(pos, dtype=np.float64)
    apriori, solved = pos0, {}

    def solve(ix):
        nonlocal apriori
        key = tuple(ix)
        if key not in solved:
            m = meas[list(ix)]
            ref = int(np.argmax(cn0_weights(m['cn0_dbhz'])))
            solved[key] = coarse_time_fix(m, ephs, float(t_gps) + int(m['sample'][ref]) / fs, apriori,
                                          code_samples=code_samples)
            if solved[key].ok and apriori is pos0:
                apriori = solved[key].ecef.copy()
        return solved[key]

    doubled = set(report.doubled)
    best, single = None, None
    for a, b in twin_sets(meas):
        fa, fb = solve(a), solve(b)
        report.assignments += 1
        for f in (fa, fb):
            if f.ok and (single is None or f.rms_m < single.rms_m):
                single = f
        if a != b and fa.ok and fb.ok and (best is None or fa.rms_m + fb.rms_m < best[0]):     # (a == b: no doubled PRN)
            best = (fa.rms_m + fb.rms_m, (fa, a), (fb, b))
    if best is None:
        fix = single if single is not None else solve(twin_sets(meas)[0][0])
        report.fixes, report.separation_m = (fix, None), None
        return fix
    (fa, a), (fb, b) = best[1], best[2]
    if have_pos:
        swap = np.linalg.norm(fb.ecef - pos0) < np.linalg.norm(fa.ecef - pos0)
    else:
        def level(ix):
            c = [meas['cn0_dbhz'][i] for i in ix if int(meas['prn'][i]) in doubled]
            return float(np.nanmean(c)) if c else 0.0
        swap = level(b) < level(a)
    if swap:
        fa, fb, a, b = fb, fa, b, a
    report.fixes, report.separation_m = (fa, fb), float(np.linalg.norm(fa.ecef - fb.ecef))
    # the records each fix is made of: what its residual test dropped is not behind it (the pair with
    # the least rms may hold a PRN the wrong way round, which either fix then drops)
    report.sets = tuple([i for i in ix if int(meas['prn'][i]) in f.prns] for f, ix in ((fa, a), (fb, b)))
    return fa


def _spoof_pass(acq, dev, n, prns, freqs, n_coh, n_seg, corr_min, f_offset, st, min_doubled):
    """_measure_pass with several candidates per PRN: pipeline.peak_candidates, refinement over
    +- one bin step (a hit's bin lies up to half a step beside a doubled satellite's Doppler, which
    the default +-120 Hz would leave at the edge of the grid), spoof_keep.
    -> (rec, found, records, SpoofReport)."""
    from .pipeline import peak_candidates, refine_centred
    cs = acq.cfg.code_samples
    pst = {}
    found = peak_candidates(acq, (dev[0], n_seg * n_coh * cs), prns, freqs, n_coh, n_seg, f_offset=f_offset,
                            corr_min=corr_min, k=SPOOF_PICKS, stats=pst)
    st['device_ms'] += pst['search_ms'] + pst['peaks_ms']
    st['peaks_ms'] = pst['peaks_ms']
    if not found:
        return None, [], np.zeros(0, MEAS_DTYPE), SpoofReport(prns=list(prns), picks=pst['picks'])
    step = abs(freqs[1] - freqs[0]) if len(freqs) > 1 else acq.cfg.step_freq
    recs, used = [], []
    for i in range(0, len(found), SPOOF_REFINE_HITS):
        f, r, ms = refine_centred(acq, dev, found[i:i + SPOOF_REFINE_HITS], f_offset=f_offset, df_half=float(step))
        st['device_ms'] += ms
        used, recs = used + f, recs + [r]
    rec = np.concatenate(recs)
    st['found'], st['refined'] = st['found'] + used, rec if st['refined'] is None else np.concatenate([st['refined'], rec])
    rec, used, out, report = spoof_keep(rec, used, cs, f_offset, min_doubled)
    report.prns, report.picks = list(prns), pst['picks']
    return rec, used, out, report


def _track_records(acq, dev, rec, out, n, f_offset, track_cfg, st):
    if len(rec):
        bits, states = acq.trackHits(dev, rec, f_offset=f_offset, **track_cfg)
        st['device_ms'] += acq.engine.last_ms()
        tracked_records(out, bits, states['bit_no'], n, acq.cfg.code_samples, track_cfg.get('pull_in_bits', 0))


def measure(acq, data, prns=None, f_offset=0.0, source=None, stats=None, cancel=None, spoof=False, antennas=None,
            beams=False, profile=False, array=False, **cfg):
    """The satellites of one snapshot: MEAS_DTYPE records, one per satellite found, sorted by PRN.

    `acq`: an acquisition.Acquisition; `data`: the samples in its input format (complex64, or the
    recorder's uint16 with raw_u8) or a (device pointer, n) pair -- host data is uploaded once and
    every stage reads that copy.  `prns`: what to search for (default acquisition.SAT_ALL; pass
    the PRNs there are ephemerides for).  Stages: pipeline.largest_peak_hits over `prns` x the
    bins (`freqs`, default the configured ones) in `n_coh`-ms segments, per PRN the largest peak
    among the bins with normMaxCorr > `corr_min`; pipeline.refine_centred; confirmed records with
    a code phase, ghosts dropped (drop_ghosts).  source 'refine': code phase and Doppler of the
    refinement record, `sample` 0.
    source 'track' (data of TRACK_MIN_SECONDS or more): Acquisition.trackHits through the same
    data, the code starts of the bits behind pull-in fitted by a line and read at the middle bit,
    `sample` there; a channel that leaves fewer than TRACK_MIN_BITS such bits keeps its refinement
    values.  source None: DEFAULT_SOURCE where it applies.  `track_cfg`: trackHits' keywords.
    `cancel`: None or False -- the stages above, once.  A C/N0 in dB-Hz (True:
    CANCEL_DBHZ) -- the records of that first pass at or above it are kept, their satellites are
    cancelled into a complex64 device copy (Acquisition.cancelHits), and the stages run again on
    the copy for every other PRN: the ghost rule of that second pass sees its own records only (the
    cancelled satellites cast no ghosts any more), and with source 'track' the kept records are
    tracked on the data as it came, the others on the copy.
    `stats`: a dict that receives device_ms (the sum of the engine's last_ms over every stage),
    found and refined (of both passes) and, with `cancel`, cancelled (the CANCEL_OUT_DTYPE records).
    `spoof` (not together with `cancel`): True -- the candidates are up to
    SPOOF_PICKS peaks per PRN (pipeline.peak_candidates), refined over +- one bin step and kept by
    spoof_keep: a PRN that is in the air twice comes back with two records.  -> (records,
    SpoofReport); `min_doubled`: the doubled PRNs that set its alarm; stats also receives spoof
    (the report) and peaks_ms.  With the option off nothing of this runs.
    `antennas` (with `spoof`, or with `array` below): A = 2 .. 8 -- `data` is [A][n] on the host, or
    (pointer, n) with A rows n samples apart behind the pointer.  Every stage above reads row 0, the
    first n samples, exactly as without the option; after spoof_keep (and tracking) the kept records'
    signatures are taken once over all rows (Acquisition.signatureHits) and spoof_resolve fills the
    report's signature, quality, rho and one_direction; stats receives signature_ms.
    `beams` (with `antennas` only): after the signatures one nulling.NullSteer of
    cfg.ngps forms a beam per kept record (beam_plan: steered at the record's signature, with a null
    at the spoofer's pooled signature where one_source finds a set and the null costs at most 3 dB)
    over the n // ngps whole blocks of the snapshot -- the tail is not beamed -- and every record is
    refined again on its own row from its own hit and, with source 'track', tracked there; a record
    whose re-refinement is not confirmed keeps its antenna-0 values.  stats receives beams_ms,
    before_beams (the records as they were) and beams (per record: prn, null carried, confirmed,
    mean gain_db, the flags seen, the weights [blocks][A]).  Without the option nothing of this runs.
    `profile` (with `spoof` only): after spoof_keep (and tracking, signatures and
    beams) every kept record's multi-tap correlation profile is taken on antenna 0
    (Acquisition.profileHits: the default taps, 20-ms runs from the record's bit edge) and
    profile_verdict fills the report's profile_t, distorted and profile; the alarm is then raised as
    well when the PRNs doubled or distorted count `min_doubled` -- a copy within the guard of the peaks shows here.  stats receives
    profile_ms.  Without the option nothing of this runs.
    `array` (with `antennas` = 2 .. 4, not together with `spoof` or `cancel`): True --
    the satellites are searched for over all rows at once, so that one no single antenna shows is
    found by the gain of the array: pipeline.array_peak_hits over `prns` x the bins, per PRN the
    largest peak over `corr_min`; the hits' signatures at their argmax and bin; one beam per hit
    steered at its signature (NullSteer.beams, no null) over the n // ngps whole blocks; refinement
    of every hit on its own beam and, with source 'track', tracking there; confirmed records, ghosts
    dropped.  A hit whose refinement on the beam is not confirmed is dropped.  stats receives array_ms,
    signature_ms, beams_ms, hits and beams (per hit: prn, confirmed, kept, mean gain_db, flags).
    Without the option nothing of this runs."""
    from .acquisition import SAT_ALL
    from .engine import CANCEL_OUT_DTYPE, DeviceBuffer
    c = acq.cfg
    cs = c.code_samples
    n_coh = int(cfg.pop('n_coh', 4))
    corr_min = float(cfg.pop('corr_min', c.corr_min))
    freqs = cfg.pop('freqs', None)
    track_cfg = dict(cfg.pop('track_cfg', None) or {})
    min_doubled = int(cfg.pop('min_doubled', SPOOF_MIN_DOUBLED))
    if cfg:
        raise TypeError(f'unknown options {sorted(cfg)}')
    if spoof and cancel not in (None, False):
        raise ValueError('spoof and cancel are not combined')
    if array and antennas is None:
        raise ValueError('array goes with antennas=A (the search combines the antennas)')
    if array and (spoof or cancel not in (None, False)):
        raise ValueError('array is not combined with spoof or cancel')
    if antennas is not None:
        if not spoof and not array:
            raise ValueError('antennas goes with spoof=True (the signatures serve the spoofing check)')
        antennas = int(antennas)
        if not 2 <= antennas <= (4 if array else 8):
            raise ValueError('antennas must be 2 .. 4' if array else 'antennas must be 2 .. 8')
    elif beams:
        raise ValueError('beams goes with antennas=A (the beams combine the antennas)')
    if profile and not spoof:
        raise ValueError('profile goes with spoof=True (the profiles serve the spoofing check)')
    if freqs is None:
        freqs = [c.min_freq + c.step_freq * i for i in range(int(round((c.max_freq - c.min_freq) / c.step_freq)))]
    prns = list(SAT_ALL if prns is None else prns)
    host = None if isinstance(data, tuple) else acq.engine._host_iq(data)
    if antennas is not None and host is not None and (host.ndim != 2 or host.shape[0] != antennas):
        raise ValueError(f'data must be [{antennas}][n], one row per antenna')
    n = int(data[1]) if host is None else host.shape[-1] if antennas is not None else host.size
    n_seg = n // cs // n_coh
    if n < min_samples(cs) or n_seg < 1:
        raise ValueError(f'{n} samples are too few: {min_samples(cs)} (40 ms and the code slide) are needed')
    can_track = n >= int(TRACK_MIN_SECONDS * 1000) * cs
    source = source or (DEFAULT_SOURCE if can_track else 'refine')
    if source not in ('refine', 'track') or (source == 'track' and not can_track):
        raise ValueError(f"source {source!r}: 'refine' or 'track', the latter from {TRACK_MIN_SECONDS} s on")
    cancel_dbhz = None if cancel is None or cancel is False else CANCEL_DBHZ if cancel is True else float(cancel)
    buf, clean, dev = None, None, data
    if host is not None:
        buf = DeviceBuffer(host.nbytes, c.device)
    try:
        if buf is not None:
            buf.upload(host)
            dev = (buf.ptr, n)
        st = {'device_ms': 0.0, 'found': [], 'refined': None}
        if array:
            out = _array_pass(acq, dev, n, prns, freqs, n_coh, n_seg, corr_min, antennas, source, f_offset, track_cfg, st)
            out = out[np.argsort(out['prn'], kind='stable')]
            if stats is not None:
                stats.update(st)
            return out
        if spoof:
            rec, found, out, report = _spoof_pass(acq, dev, n, prns, freqs, n_coh, n_seg, corr_min, f_offset, st,
                                                  min_doubled)
            if source == 'track' and len(out):
                _track_records(acq, dev, rec, out, n, f_offset, track_cfg, st)     # (indexed by record)
            if antennas is not None:
                report.antennas = antennas
                if len(out):
                    cov, _ = acq.signatureHits(dev, out, antennas, f_offset=f_offset)
                    st['signature_ms'] = acq.engine.last_ms()
                    st['device_ms'] += st['signature_ms']
                    v, report.quality = signature_vectors(cov)
                    spoof_resolve(report, out, None, v)
                    if beams:
                        _beam_pass(acq, dev, n, found, out, cov, v, report.rho, antennas, source, freqs, f_offset,
                                   track_cfg, st)
                else:
                    st['signature_ms'] = 0.0
            if profile:
                st['profile_ms'] = 0.0
                if len(out):
                    pcov, runs = acq.profileHits((dev[0], n), out, f_offset=f_offset)
                    st['profile_ms'] = acq.engine.last_ms()
                    st['device_ms'] += st['profile_ms']
                    profile_verdict(report, out, pcov, runs, cs, 8 if cs == 2048 else 32, min_doubled)
            st['spoof'] = report
            if stats is not None:
                stats.update(st)
            return out, report
        rec, found, out = _measure_pass(acq, dev, n, prns, freqs, n_coh, n_seg, corr_min, f_offset, st)
        if cancel_dbhz is not None:
            st['cancelled'] = np.zeros(0, CANCEL_OUT_DTYPE)
            strong = out['cn0_dbhz'] >= cancel_dbhz                   # (NaN: no)
        if cancel_dbhz is None or not strong.any():
            if source == 'track' and len(out):
                _track_records(acq, dev, rec, out, n, f_offset, track_cfg, st)
        else:
            rec, out = rec[strong], out[strong]
            if source == 'track':
                _track_records(acq, dev, rec, out, n, f_offset, track_cfg, st)
            clean = DeviceBuffer(8 * n, c.device)
            _, st['cancelled'] = acq.cancelHits(dev, rec, f_offset=f_offset, out=clean.ptr)
            st['device_ms'] += acq.engine.last_ms()
            kept = set(out['prn'].tolist())
            rest = [p for p in prns if p not in kept]
            was_raw = acq.engine.raw_u8
            rec2, out2 = None, np.zeros(0, MEAS_DTYPE)
            try:                                     # the copy is complex64 whatever the data is
                if was_raw:
                    acq.engine.set_input_format(False)
                dev2 = (clean.ptr, n)
                if rest:
                    rec2, _, out2 = _measure_pass(acq, dev2, n, rest, freqs, n_coh, n_seg, corr_min, f_offset, st)
                if source == 'track' and len(out2):
                    _track_records(acq, dev2, rec2, out2, n, f_offset, track_cfg, st)
            finally:
                if was_raw:
                    acq.engine.set_input_format(True)
            out = np.concatenate([out, out2])
        out = out[np.argsort(out['prn'], kind='stable')]
        if stats is not None:
            stats.update(st)
        return out
    finally:
        if buf is not None:
            buf.free()
        if clean is not None:
            clean.free()


# ---------------------------------------------------------------- collective detection
COLLECTIVE_POOL = 8                      # lags pooled at the coarsest level of the pyramid
COLLECTIVE_ELEVATION = 5.0               # degrees above the a-priori horizon a PRN must stand to be searched
COLLECTIVE_WINDOW_MIN = 4.0              # (S - mean) / std a satellite's 3 x 3 window must reach
COLLECTIVE_MARGIN_MIN = 6.0              # (best - median) / robust sigma of the coarsest map
COLLECTIVE_FINE = 5                      # grid points per axis of the levels after the first


def enu_axes(pos):
    """Unit vectors east, north and up at ECEF `pos` (geodetic)."""
    lat, lon, _ = P.ecef_to_geo(np.asarray(pos, dtype=np.float64))
    la, lo = np.radians(lat), np.radians(lon)
    east = np.array([-np.sin(lo), np.cos(lo), 0.0])
    north = np.array([-np.sin(la) * np.cos(lo), -np.sin(la) * np.sin(lo), np.cos(la)])
    return east, north, np.cross(east, north)


def collective_model(ephs, prns, t_gps, pos, cs, f_offset=0.0):
    """What a receiver at ECEF `pos` at GPS time `t_gps` (that of the first sample) expects of
    `prns`, as collective detection needs it: the code start of satellite p lies at lag
        lag0_p + g_e_p E + g_n_p N + g_t_p T + clock      (mod cs)
    for a receiver E metres east and N metres north of `pos` at time t_gps + T.  lag0 = fs / c *
    modelled_range mod cs; g_e, g_n = fs / c * the line of sight's east and north components;
    g_t = fs / c * the range rate.  The part of the time that all satellites share (-fs T) and the
    receiver's clock bias are the common term `clock`.
    -> dict of arrays per PRN: lag0, g_e, g_n, g_t, f_hz (the predicted Doppler plus f_offset),
    elevation (degrees)."""
    fs = 1000.0 * cs
    east, north, up = enu_axes(pos)
    t = np.full(len(prns), float(t_gps))
    f, e, fd = _model(ephs, prns, t, np.asarray(pos, dtype=np.float64))
    k = fs / P.GPS_C
    return {'lag0': np.mod(k * f, cs), 'g_e': k * (e @ east), 'g_n': k * (e @ north), 'g_t': k * fd,
            'f_hz': -fd * L1_HZ / P.GPS_C + f_offset, 'elevation': np.degrees(np.arcsin(-(e @ up)))}


def collective_levels(radius_m, time_s, cs, g_t_max, pool=COLLECTIVE_POOL):
    """The pyramid: per level (pool w, step in metres, step in seconds, points per horizontal axis,
    points in time).  w halves from `pool` to 1; the horizontal step is half of w samples of range
    (w * c / fs / 2: neighbouring points then differ by at most 0.71 w lags in any satellite, less
    than the w lags a pooled row covers), the time step a quarter of w lags of the fastest
    satellite.  The first level covers +-radius_m and +-time_s, the others +-2 steps of their own
    around the best cell of the level before (which is within one step of theirs)."""
    fs = 1000.0 * cs
    out, w = [], int(pool)
    while w >= 1:
        step_m, step_t = 0.5 * w * P.GPS_C / fs, 0.25 * w / max(g_t_max, 1.0e-3)
        if not out:
            n_h, n_t = 2 * int(np.ceil(radius_m / step_m)) + 1, 2 * int(np.ceil(time_s / step_t)) + 1
        else:
            n_h = n_t = COLLECTIVE_FINE
        out.append((w, step_m, step_t, n_h, n_t))
        w //= 2
    return out


def collective_level_args(model, bins, level):
    """The satellites (engine.COLLECTIVE_SAT_DTYPE) and the grid (a dict) of one level, centred on
    the point `model` was formed at.  `bins`: per satellite (row, bin_lo, bin_hi).  A pooled row
    holds the maximum of lags l .. l + w - 1, so the prediction is moved back by (w - 1) / 2."""
    from ._lib import COLLECTIVE_SAT_DTYPE
    w, step_m, step_t, n_h, n_t = level
    sats = np.zeros(len(bins), COLLECTIVE_SAT_DTYPE)
    sats['row'], sats['bin_lo'], sats['bin_hi'] = np.array(bins, dtype=np.int64).T
    sats['lag0'] = model['lag0'] - 0.5 * (w - 1)
    sats['g_e'], sats['g_n'], sats['g_t'] = model['g_e'], model['g_n'], model['g_t']
    grid = dict(n_e=n_h, n_n=n_h, n_t=n_t, pool=w, e0=-0.5 * (n_h - 1) * step_m, n0=-0.5 * (n_h - 1) * step_m,
                t0=-0.5 * (n_t - 1) * step_t, d_e=step_m, d_n=step_m, d_t=step_t)
    return sats, grid


def collective_best(cells, grid):
    """The best cell of a map.  Rounding the predicted lags to whole samples leaves a plateau of
    equal scores around the optimum: of the cells that hold the largest score, the one nearest to
    their centroid (in cells; the first of equally near ones in (i_t, i_n, i_e) order).
    -> (E, N, T, clock lag, score, index)."""
    top = np.argwhere(cells['score'] == cells['score'].max())
    d = top - top.mean(axis=0)
    it, i_n, ie = (int(v) for v in top[int(np.argmin(np.sum(d * d, axis=1)))])
    return (grid['e0'] + ie * grid['d_e'], grid['n0'] + i_n * grid['d_n'], grid['t0'] + it * grid['d_t'],
            int(cells['lag'][it, i_n, ie]), float(cells['score'][it, i_n, ie]), (it, i_n, ie))


def collective_margin(cells):
    """(best - median) / (1.4826 * median absolute deviation) of a map's scores."""
    sc = cells['score'].astype(np.float64).ravel()
    med = np.median(sc)
    return float((sc.max() - med) / max(1.4826 * np.median(np.abs(sc - med)), 1.0e-30))


def collective_pyramid(cell_map, ephs, prns, bins, t_gps, pos, cs, radius_m, time_s, f_offset=0.0,
                       pool=COLLECTIVE_POOL):
    """The coarse-to-fine search.  `cell_map(sats, grid)` -> the cell map of one level
    (AcqEngine.collective on the GPU).  Every level is linearised anew at the best point of the one
    before.  -> dict: ecef, t_gps, lag (clock, samples), score, margin (of the coarsest map), map
    and grid (of the last level), model (collective_model at the optimum), levels (per level: pool,
    grid shape, best index, score, grid, and the centre (ecef, t_gps) its offsets count from)."""
    pos, t = np.array(pos, dtype=np.float64), float(t_gps)
    model = collective_model(ephs, prns, t, pos, cs, f_offset)
    levels = collective_levels(radius_m, time_s, cs, float(np.abs(model['g_t']).max()), pool)
    res = {'levels': []}
    for k, level in enumerate(levels):
        if level[3] * level[3] * level[4] > (1 << 22):
            raise ValueError(f'the first level has {level[3]} x {level[3]} x {level[4]} points, more than one '
                             'collective call takes: a smaller radius_m or time_s')
        sats, grid = collective_level_args(model, bins, level)
        cells = cell_map(sats, grid)
        E, N, T, lag, score, idx = collective_best(cells, grid)
        if k == 0:
            res['margin'] = collective_margin(cells)
        res['levels'].append({'pool': level[0], 'shape': cells.shape, 'best': idx, 'score': score, 'grid': grid,
                              'centre': (pos.copy(), t)})
        east, north, _ = enu_axes(pos)
        pos, t = pos + E * east + N * north, t + T
        # the clock lag counts from the prediction this level was given; the next one (or the
        # caller) gets it relative to the new linearisation
        here = sats['lag0'] + sats['g_e'] * E + sats['g_n'] * N + sats['g_t'] * T + lag + 0.5 * (level[0] - 1)
        model = collective_model(ephs, prns, t, pos, cs, f_offset)
        clock = here - model['lag0']
        clock = clock[0] + np.mod(clock - clock[0] + cs / 2.0, cs) - cs / 2.0      # (one turn of the code for all)
        res.update(map=cells, grid=grid, score=score)
    res.update(ecef=pos, t_gps=t, model=model, lag=float(np.mod(np.median(clock), cs)))
    return res


def collective_records(rows_of, prns, freqs, model, lag, cs, window_min=COLLECTIVE_WINDOW_MIN):
    """Measurements at the optimum of a collective search.  rows_of(p) -> the surfaces of
    satellite p in its bins, float [bins, cs]; freqs[p] their frequencies; the predicted lag of p
    is model['lag0'][p] + lag.  Per satellite the largest of the 3 lags around the prediction, in
    the bin where it is largest, counts as a measurement if its (S - mean) / std (mean and std of
    its bin's whole row) reaches `window_min` -- lower than the threshold of a search over the
    whole surface, because 3 lags x the satellite's bins are searched, not 2048 x 51 cells.  The
    sub-sample phase is the vertex of the parabola through the peak and its two neighbours, within
    half a sample.  -> MEAS_DTYPE records (sample 0, cn0_dbhz NaN: nothing here measures it,
    source b'collec'), and the (S - mean) / std of every satellite."""
    out, zs = [], np.zeros(len(prns))
    for p, prn in enumerate(prns):
        S_ = np.asarray(rows_of(p), dtype=np.float64)
        z = (S_ - S_.mean(axis=1, keepdims=True)) / np.where(S_.std(axis=1, keepdims=True) > 0,
                                                              S_.std(axis=1, keepdims=True), np.inf)
        l0 = int(np.floor(model['lag0'][p] + lag + 0.5))
        lags = np.array([l0 - 1, l0, l0 + 1]) % cs
        b, j = np.unravel_index(int(np.argmax(z[:, lags])), (len(z), 3))
        zs[p] = z[b, lags[j]]
        if zs[p] < window_min:
            continue
        l = int(lags[j])
        lo, mid, hi = S_[b, (l - 1) % cs], S_[b, l], S_[b, (l + 1) % cs]
        den = lo - 2.0 * mid + hi
        frac = float(np.clip(0.5 * (lo - hi) / den, -0.5, 0.5)) if den < 0 else 0.0
        out.append((int(prn), 0, (l + frac) % cs, float(freqs[p][b]), np.nan, np.nan, b'collec'))
    return np.array(out, dtype=MEAS_DTYPE), zs


def collective_plan_bins(ephs, t_gps, pos, cfg, f_offset=0.0, elevation=COLLECTIVE_ELEVATION):
    """Which PRNs a collective search takes and where: those of `ephs` standing `elevation`
    degrees above the a-priori horizon, each with the window of its predicted Doppler bin +-1 on
    the configured bin grid.  -> (prns, freqs searched (sorted, the union of the windows), per
    satellite (row, bin_lo, bin_hi) into them)."""
    prns = sorted(int(p) for p in ephs)
    m = collective_model(ephs, prns, t_gps, pos, cfg.code_samples, f_offset)
    nb = int(round((cfg.max_freq - cfg.min_freq) / cfg.step_freq))
    seen = [(p, int(np.clip(round((f - cfg.min_freq) / cfg.step_freq), 0, nb - 1)))
            for p, f, el in zip(prns, m['f_hz'], m['elevation']) if el >= elevation]
    used = sorted({b for _, c in seen for b in range(max(c - 1, 0), min(c + 1, nb - 1) + 1)})
    freqs = [cfg.min_freq + cfg.step_freq * b for b in used]
    bins = [(r, used.index(max(c - 1, 0)), used.index(min(c + 1, nb - 1))) for r, (_, c) in enumerate(seen)]
    return [p for p, _ in seen], freqs, bins


def collective_search(acq, data, ephs, t_gps, pos, f_offset=0.0, radius_m=15.0e3, time_s=2.0, stats=None, **cfg):
    """Collective detection: no decision per satellite -- the deep surfaces of
    all visible satellites are added at the lags a candidate (position, coarse time, clock)
    predicts, and the candidate where the sum peaks is taken; satellites that are each under the
    search's threshold add up.

    `pos`, `t_gps`: the a-priori ECEF position and the GPS time of the first sample, believed
    within `radius_m` (horizontally) and `time_s`.  The height stays at the a-priori's: the search
    moves east and north only.  1. collective_plan_bins picks the PRNs and their bin windows.  2. One
    deep search with rows over them (`n_coh`-ms segments).  3. collective_pyramid: levels of pooled
    rows from `pool` samples down to 1, each linearised at the best cell of the one before.  4. The
    best (position, time, clock lag), the score map of the last level, the margin of the peak of
    the coarsest map, and collective_records' measurements at the optimum (`window_min`).
    -> dict of collective_pyramid's entries plus prns, meas, z (per PRN), device_ms (all calls) and
    level_ms (per level)."""
    c = acq.cfg
    cs = c.code_samples
    n_coh = int(cfg.pop('n_coh', 4))
    pool = int(cfg.pop('pool', COLLECTIVE_POOL))
    window_min = float(cfg.pop('window_min', COLLECTIVE_WINDOW_MIN))
    elevation = float(cfg.pop('elevation', COLLECTIVE_ELEVATION))
    if cfg:
        raise TypeError(f'unknown options {sorted(cfg)}')
    n = int(data[1]) if isinstance(data, tuple) else len(data)
    n_seg = n // cs // n_coh
    if n_seg < 1:
        raise ValueError(f'{n} samples hold no segment of {n_coh} code periods')
    prns, freqs, bins = collective_plan_bins(ephs, t_gps, pos, c, f_offset, elevation)
    if not prns:
        raise ValueError('no satellite of the ephemerides stands above the a-priori horizon')
    _, rows = acq.deepRows(data if isinstance(data, tuple) else acq.engine._host_iq(data), prns, freqs, n_coh,
                           n_seg, f_offset=f_offset)
    try:
        ms = {'device_ms': acq.engine.last_ms(), 'level_ms': []}

        def cell_map(sats, grid):
            cells = acq.engine.collective(rows, sats, grid, nsv_rows=len(prns), nbins=len(freqs))
            ms['level_ms'].append(acq.engine.last_ms())
            return cells
        res = collective_pyramid(cell_map, ephs, prns, bins, t_gps, pos, cs, radius_m, time_s, f_offset, pool)
        host = rows.download(np.float32, len(prns) * len(freqs) * cs).reshape(len(prns), len(freqs), cs)
    finally:
        rows.free()
    res['meas'], res['z'] = collective_records(
        lambda p: host[bins[p][0], bins[p][1]:bins[p][2] + 1], prns,
        [freqs[b[1]:b[2] + 1] for b in bins], res['model'], res['lag'], cs, window_min)
    res.update(prns=prns, level_ms=ms['level_ms'], device_ms=ms['device_ms'] + sum(ms['level_ms']))
    if stats is not None:
        stats['collective'] = res
    return res


def _collective_fix(acq, data, ephs, t_gps, pos, f_offset, cfg, stats):
    """collective_search, then coarse_time_fix on its measurements from its optimum."""
    res = collective_search(acq, data, ephs, t_gps, pos, f_offset=f_offset, stats=stats, **cfg)
    meas = res['meas']
    if res['margin'] < COLLECTIVE_MARGIN_MIN:
        fix = Fix(reason=f"collective peak {res['margin']:.1f} robust sigma above the map, "
                         f'{COLLECTIVE_MARGIN_MIN} needed')
    elif len(meas) < MIN_SAT:
        fix = Fix(reason=f'{len(meas)} satellites measured at the collective optimum, {MIN_SAT} needed')
    else:
        fix = coarse_time_fix(meas, ephs, res['t_gps'], res['ecef'], code_samples=acq.cfg.code_samples)
    fix.path = 'collective'
    return fix, meas, res['device_ms']


def snapshot_fix(acq, data, ephs, t_gps, pos=None, f_offset=0.0, source=None, cancel=None, stats=None,
                 collective=None, collective_cfg=None, spoof=False, antennas=None, beams=False, profile=False,
                 array=False, **cfg):
    """measure -> (doppler_fix when `pos` is None) -> coarse_time_fix.  `t_gps`: the GPS seconds
    of week of the first sample as far as known; `cancel`, `stats`: measure's.  -> (Fix,
    measurements, device ms).  The Fix's t_gps is that of its `sample`.
    `collective` (needs `pos`): True -- when measure yields fewer than MIN_SAT
    satellites, collective_search (keywords: `collective_cfg`) supplies the a-priori and the
    measurements instead, and coarse_time_fix solves from them; 'always' -- it does so whatever
    measure yields.  Fix.path says which of the two made the fix.  None or False: nothing of this
    runs.
    `spoof` (not together with `cancel` or `collective`): True -- measure(...,
    spoof=True); without a doubled PRN everything goes on as with the option off.  With doubled
    PRNs twin_fixes solves once per consistent assignment of their records to two sets; the first
    return value is fix_a, the SpoofReport (doubled, alarm, fixes = (fix_a, fix_b), separation_m)
    rides on stats['spoof'] and on the Fix's attribute `spoof`.  With one antenna which fix is
    authentic is not claimed.
    `antennas` (with `spoof` only, measure's): twin_fixes is followed by
    spoof_resolve on the records' signatures; with a verdict the authentic fix goes first
    (fixes[0], the returned Fix, report.authentic 0) whatever the a-priori or the C/N0 say, without
    one the order of twin_fixes stands.  report.one_direction raises the alarm without a doubled
    PRN.
    `beams` (with `antennas` only): measure's -- the records the fixes are made of
    were measured on their own beams.
    `profile` (with `spoof` only): measure's -- report.distorted and profile_t, and an
    alarm that is raised as well when the PRNs doubled or distorted count `min_doubled`; the fixes are
    made as without it.
    `array` (with `antennas` = 2 .. 4, without `spoof`, `cancel`, `beams` and
    `collective`): measure's -- the satellites are found over all antennas at once and measured on
    their own beams."""
    if array and (antennas is None or spoof or beams or profile or collective):
        raise ValueError('array goes with antennas=A alone (not with spoof, beams, profile or collective)')
    if collective not in (None, False, True, 'always'):
        raise ValueError(f"collective {collective!r}: None, False, True or 'always'")
    if collective and pos is None:
        raise ValueError('collective detection needs an a-priori position')
    if spoof and collective:
        raise ValueError('spoof and collective are not combined')
    if antennas is not None and not spoof and not array:
        raise ValueError('antennas goes with spoof=True (the signatures serve the spoofing check)')
    if beams and antennas is None:
        raise ValueError('beams goes with antennas=A (the beams combine the antennas)')
    if profile and not spoof:
        raise ValueError('profile goes with spoof=True (the profiles serve the spoofing check)')
    stats = {} if stats is None else stats
    report = None
    if spoof:
        meas, report = measure(acq, data, prns=sorted(ephs), f_offset=f_offset, source=source, stats=stats,
                               cancel=cancel, spoof=True, antennas=antennas, **({'beams': True} if beams else {}),
                               **({'profile': True} if profile else {}), **cfg)
    else:
        meas = measure(acq, data, prns=sorted(ephs), f_offset=f_offset, source=source, stats=stats, cancel=cancel,
                       **({'antennas': antennas, 'array': True} if array else {}), **cfg)
    ms = stats.get('device_ms', 0.0)
    if report is not None and report.doubled:
        if len(set(meas['prn'].tolist())) < MIN_SAT:
            fix = Fix(reason=f"{len(set(meas['prn'].tolist()))} satellites measured, {MIN_SAT} needed")
        else:
            have_pos = pos is not None
            if not have_pos:                         # (one record per PRN, the stronger: a Doppler is a Doppler)
                pos, _ = doppler_fix(meas[twin_sets(meas)[0][0]], ephs, t_gps, f_offset=f_offset)
            fix = twin_fixes(meas, ephs, t_gps, pos, report, acq.cfg.code_samples, have_pos)
            if report.signature is not None:
                spoof_resolve(report, meas, report.sets, report.signature)
                fix = authentic_first(report)
        fix.spoof = report
        return fix, meas, ms
    if collective and (collective == 'always' or len(meas) < MIN_SAT):
        fix, meas, cms = _collective_fix(acq, data, ephs, t_gps, pos, f_offset, dict(collective_cfg or {}), stats)
        return fix, meas, ms + cms
    if len(meas) < MIN_SAT:
        return Fix(reason=f'{len(meas)} satellites measured, {MIN_SAT} needed'), meas, ms
    fs = 1000.0 * acq.cfg.code_samples
    if pos is None:
        pos, _ = doppler_fix(meas, ephs, t_gps, f_offset=f_offset)
    ref = int(np.argmax(cn0_weights(meas['cn0_dbhz'])))
    fix = coarse_time_fix(meas, ephs, float(t_gps) + int(meas['sample'][ref]) / fs, pos,
                          code_samples=acq.cfg.code_samples)
    if report is not None:
        report.fixes = (fix, None)
        fix.spoof = report
    return fix, meas, ms
