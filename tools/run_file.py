#!/usr/bin/env python3
"""A recording in, position fixes out: the reference's file mode (README.md:177-187,
gpsglob.LIVE_MEAS = False / BIN_DATA; gpsrecv.streamData -> processData -> UDP / pickle ->
gpseval) as one command on the GPU path.

    python tools/run_file.py <recording.bin> [--seconds S] [--start-stream K] [--save-pickle P]
                             [--ephemeris gpsEphem.json] [--cpu-acq] [--excise] [--sweep [L]] [--blank] [--json]
                             [--antenna FILE ... --null [--null-taps T]]
                             [--format FMT --fs HZ --if HZ --conjugate] [--deep-acq SECONDS [--refine [--track [--weak-fix]]]]
                             [--save-ephemeris PATH] [--snapshot SECONDS --ephemeris E --time T [--near LAT,LON[,H]] [--cancel [DBHZ]] [--collective [RADIUS_KM]] [--spoof-check [K] [--profile-check]] [--antenna FILE ... [--beams]]] [--antenna FILE ... --array-search]]

    <recording.bin>   what gpsbin.py records and streamData reads (gpsrecv.py:162-173):
                      little-endian uint16 per sample, low byte I, high byte Q, 2.048 Msps
                      (1 min = 245.76 MB).  `data/test.bin` of the reference when it is there.

Flow: ingest.open_blocks (read_raw_blocks: the file loop of streamData, START_STREAM honoured) ->
pipeline.Receiver(raw_u8=True).feed (cold sweep, channel selection, tracking, hand-off
datagrams; the u8 decode happens inside the GPU kernels) -> position.PositionSolver.feed
(prepCodePhase ... leastSquaresPos, the evaluation side's data path) -> fixes; the mean of
the second half of the fixes is printed as latitude / longitude / height.  --save-pickle
writes the datagram list exactly as SAVE_PICKLE does (gpsrecv.py:205-212): an unmodified
gpseval.py replays it with LOAD_PICKLE.  --cpu-acq times BASELINE configs[0] beside it: the
cold acquisition of the reference's numpy path (oracle restatement, test infrastructure) on
the first five blocks of the same file, on one host core.  --excise removes narrowband
interference (continuous-wave tones) from every block on the GPU before the receiver sees it
(pipeline.Receiver(excise=True)).  --blank zeroes pulsed and swept (chirp)
interference sample by sample on the GPU (pipeline.Receiver(blank=True)); with
--excise the tones are removed first, then the pulses.  --sweep [L] removes swept and chirp
interference in the time-frequency plane of frames of L samples (default: the library's, 64) on the GPU
(pipeline.Receiver(sweep=True)), between --excise and --blank; the report gains
'sweep': the blocks excised and passed through and the mean share of the plane removed.
--antenna FILE (repeatable) names the files
of the further channels of a coherent multi-antenna recorder, sample-aligned with the recording
(antenna 0, the reference element), and --null combines them by null steering on the GPU ahead of
everything else (pipeline.Receiver(antennas=A, null=True)): a defence against
jammers that are wide in frequency and continuous in time; the flag (1 nulled, 0 antenna 0 passed
through) and the predicted gain of every block are printed, with --json under 'null'; --null-taps T
(3, 5 or 7) gives every antenna T space-time taps instead of one weight.  --format (c64, u8iq, sc8, sc16, r8), --fs (the
input rate in Hz), --if (the IF of real input or the tuner offset of complex input, Hz) and
--conjugate read a recording of another front end: frontend.FrontEnd decodes, mixes, filters and
resamples it on the GPU to complex64 blocks at 2.048 Msps, which Receiver(raw_u8=False) takes
(DESIGN.md 4.2c); --start-stream then skips output blocks.  Without them the path above is unchanged.
--deep-acq SECONDS adds a second acquisition pass at the end, over the first SECONDS of the recording
and for the PRNs the 4-ms sweep did not acquire: Acquisition.sweepDeepSats, the non-coherent search
with the code Doppler compensated.  It prints PRN, Doppler bin, code delay and
normMaxCorr of what it finds and changes nothing else: the satellites are not handed to tracking.
--refine (with --deep-acq) refines what the second pass found on the same data: Acquisition.refineHits
 integrates coherently over each 20-ms data bit and prints the fine Doppler, the bit
edge, the sub-sample code phase, C/N0 and its own detection ratio per satellite -- what a tracking
channel of the reference's kind would be opened with (acquisition.hit_at).
--track (with --refine) opens a bit-synchronous tracking channel on every confirmed hit
(Acquisition.trackHits / AcqEngine.track_weak) and follows it through the recording in
chunks: 20-ms coherent sums between the bit edges refinement found, carrier and code loops closed at
50 Hz.  It prints, per PRN, the bits tracked, the Doppler (mean of the last 20 bits), the code phase,
C/N0 and the phase-lock indicator at the end, and the device time.
--weak-fix (with --track) runs the receiver inside pipeline.WeakAssist: the same
search, refinement and tracking, online, on the first SECONDS behind the cold sweep; the weak
channels' subframes and code phases are merged into the datagrams the position fix is made of (and
--save-pickle writes).  The report gains, per weak PRN, the subframes decoded and the fixes it took
part in.  Without the flag every output is as before.
--save-ephemeris PATH writes the ephemerides the run decoded in the format --ephemeris reads.
--snapshot SECONDS replaces the run above by a snapshot fix (gpsmi.snapshot): the first
SECONDS behind --start-stream (from 0.043 s on), read through --format / --fs / --if, --excise and --blank as
above, searched, refined and -- from 0.5 s on -- tracked on the GPU for the PRNs of --ephemeris, and a
position solved from the code phases without a decoded subframe.  It needs --time, the time of the first
sample read, within 30 s: GPS seconds of week, or a UTC timestamp (2024-05-01T12:00:00) converted with the
leap seconds of position.LEAPSEC and the ephemerides' week; --near LAT,LON[,H] is the position as far as
known (within 50 km), without it the Dopplers give one.  It prints the measurements, the fix and the
device time; with --json one line with a 'snapshot' key.  --cancel [DBHZ] (with --snapshot only): the
satellites measured at or above DBHZ (default 40 dB-Hz) are cancelled from the samples and the others
measured on what is left; the report gains a 'cancelled' list.  Without the flag every
output is as before.  --collective [RADIUS_KM] (with --snapshot and --near): when fewer than five satellites
are measured, position, coarse time and clock are searched collectively within RADIUS_KM (default 15 km)
and 2 s of --near and --time, and the fix is solved from the satellites measured at that optimum
(DESIGN.md 4.2k); the report gains 'path' and, where the search ran, a 'collective' entry.
--spoof-check [K] (with --snapshot only): up to four peaks per PRN are refined, PRNs that are in the air twice
are listed, from K of them on (default 2) the alarm is raised, and both sets of records are solved: the
report gains a 'spoof' entry with the doubled PRNs, both fixes and their separation.  With one
antenna which fix is authentic is not decided, and the exit status is 0 either way.  With --antenna FILE ...
(without --null) every file gives one further row of the snapshot of a coherent multi-antenna recorder: every
record gets a spatial signature over the antennas, the set of doubled records that all arrive from one direction
is the spoofer's, and the report names the authentic fix (first) and says whether every signal arrives from one
direction ('authentic', 'one_source', 'one_direction').  --beams on top of that measures every
record again on a beam of its own over the antennas, steered at its signature and with a null at the spoofer
where one is found and the null costs at most 3 dB; the report gains a 'beams' entry with one line per record
(the null, the predicted gain, C/N0 on antenna 0).  --array-search (with --snapshot and one to three --antenna FILE, without --spoof-check) searches for the satellites
over all antennas at once (gpsmi_acq_search_array) and measures every hit on a beam of its own: a
four-antenna recording then finds what no single antenna shows; the report names the satellites antenna 0 alone would
have found beside those of the array.  --profile-check (with --spoof-check; one
antenna is enough) takes every record's multi-tap correlation profile and tests whether one code replica
explains it: a copy within two chips of the authentic code, which the peaks cannot separate, shows as a
distorted profile; such PRNs are listed ('distorted') and count towards the alarm like doubled ones, and the
report gains one 'profile' line per record.

There is no recording in this repository (data/test.bin is absent from the reference
checkout, SURVEY F2, and too short for a fix even upstream): tests/test_run_file.py writes a
synthetic one with gpsmi.synth_nav and checks the fix this command prints."""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gps-sdr-receiver_amd'))


def cpu_cold_acquisition(path, n_blocks=5):
    """BASELINE configs[0]: 31 SV x 50 bins x 4 ms first-hit sweep of the reference's numpy path
    on the first blocks of the file, one core (the oracle: checker / CPU baseline only)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import gps_oracle as orc
    from gpsmi import ingest, synth
    p = orc.Params()
    t = orc.sec_time(p)
    spectra = {s: orc.fft_cacode(s) for s in range(2, 33)}
    blocks = []
    for raw in ingest.read_raw_blocks(path):
        blocks.append(synth.raw_to_c64(raw))
        if len(blocks) == n_blocks:
            break
    t0 = time.perf_counter()
    sat_lst, found, freq = list(range(2, 33)), [], p.min_freq
    for blk in blocks:
        ready, freq, found = orc.sweep_all_sats(blk, freq, sat_lst, found, p.it_sweep_all, p, spectra, t)
    return {'wall_ms': round((time.perf_counter() - t0) * 1e3, 1), 'cores': 1, 'blocks': len(blocks),
            'found': [(int(s), float(f), int(d)) for _, s, f, d in found]}


TRACK_CHUNK_BLOCKS = 16


def track_refined(acq, rec, whole, source, cfg):
    """--track: channels on the confirmed records of refineHits, followed through `whole` (the data
    they were refined on, stream index 0) and the blocks `source` still yields, in chunks of
    TRACK_CHUNK_BLOCKS blocks (pipeline.WeakTracker)."""
    from gpsmi.acquisition import open_weak_channels
    from gpsmi.pipeline import WeakTracker
    cs = cfg.code_samples
    good = rec[(rec['confirmed'] == 1) & (rec['code_phase'] >= 0)]
    if not len(good):
        return {'device_ms': 0.0, 'chunks': 0, 'channels': []}
    trk = WeakTracker(acq.engine, open_weak_channels(good, cfg))
    hist = [[] for _ in good]                       # (f_hz, cn0, lock) of every bit
    step = TRACK_CHUNK_BLOCKS * cfg.ngps

    def chunks():
        for pos in range(0, len(whole), step):
            yield whole[pos:pos + step]
        while True:
            got = [b for _, b in zip(range(TRACK_CHUNK_BLOCKS), source)]
            yield np.concatenate(got) if got else whole[:0]
            if len(got) < TRACK_CHUNK_BLOCKS:
                return

    for data in chunks():
        for h, bits in enumerate(trk.push(data)):
            hist[h] += [(float(r['f_hz']), float(r['cn0_dbhz']), float(r['lock'])) for r in bits]
    states, ms, chunks = trk.states, trk.device_ms, trk.chunks
    chans = []
    for h, st in enumerate(states):
        f = [x[0] for x in hist[h][-20:]]
        cn0 = hist[h][-1][1] if hist[h] else float('nan')
        chans.append({'prn': int(st['prn']), 'bits': int(st['bit_no']),
                      'f_hz': round(float(np.mean(f)), 2) if f else round(float(st['f_hz']), 2),
                      'code_phase': round(float(st['tau'] % cs), 3),
                      'cn0_dbhz': None if np.isnan(cn0) else round(cn0, 2),
                      'lock': round(hist[h][-1][2], 3) if hist[h] else 0.0})
    return {'device_ms': round(ms, 3), 'chunks': chunks, 'channels': chans}


def deep_acquisition(path, seconds, start_stream, skip_prns, frontend=None, n_coh=4, refine=False, track=False):
    """--deep-acq: Acquisition.sweepDeepSats (code-Doppler-compensated non-coherent search, DESIGN.md
    4.2e) over the first `seconds` of the recording, n_coh-ms segments, the reference's 50 bins, for
    the PRNs not in `skip_prns`.  refine: the hits are refined on the blocks read
    (Acquisition.refineHits) and reported under 'refined'; track: the confirmed ones
    are then tracked through the rest of the recording (track_refined) and reported under 'tracked'.
    Nothing is handed to the receiver's own tracking."""
    from gpsmi import ingest
    from gpsmi.acquisition import Acquisition, SAT_ALL
    from gpsmi.engine import Config
    cfg = Config()
    n_seg = int(round(seconds * 1000)) // n_coh
    if not 1 <= n_seg <= 32768:
        sys.exit(f'--deep-acq: {n_coh}-ms segments of {seconds} s: {n_seg}, must be 1..32768')
    need = n_seg * n_coh * cfg.code_samples
    with ingest.open_blocks(path, cfg, start_stream, frontend) as (source, raw_u8):
        blocks, have = ingest.take(source, need)
        if have < need:
            sys.exit(f'--deep-acq: the recording holds {have} samples after stream {start_stream}, '
                     f'{seconds} s need {need}')
        whole = np.concatenate(blocks)
        data = whole[:need]
        acq = Acquisition(cfg, raw_u8=raw_u8)
        freqs = [cfg.min_freq + cfg.step_freq * i
                 for i in range(int(round((cfg.max_freq - cfg.min_freq) / cfg.step_freq)))]
        sat_lst = [s for s in SAT_ALL if s not in skip_prns]
        res = acq.sweepDeepSats(data, freqs, sat_lst, [], n_coh=n_coh, n_seg=n_seg)
        ms = acq.engine.last_ms()
        out = {'seconds': n_seg * n_coh / 1000.0, 'n_coh': n_coh, 'n_seg': n_seg, 'device_ms': round(ms, 3),
               'searched': sat_lst,
               'found': [(int(s), float(f), int(d), round(float(nmc), 2)) for nmc, s, f, d in res]}
        if refine and res:
            if len(whole) < 43 * cfg.code_samples:
                sys.exit(f'--refine: {len(whole)} samples are too few for 40 ms and the code slide')
            rec = acq.refineHits(whole, res)
            out['refined'] = {'n_ms': int(20 * (rec['n_bits'][0] + 1)), 'device_ms': round(acq.engine.last_ms(), 3),
                              'records': [{'prn': int(r['prn']), 'f_hz': round(float(r['f_hz']), 2),
                                           'edge_ms': int(r['edge_ms']), 'code_phase': round(float(r['code_phase']), 3),
                                           'cn0_dbhz': None if np.isnan(r['cn0_dbhz']) else round(float(r['cn0_dbhz']), 2),
                                           'ratio': round(float(r['ratio']), 3), 'confirmed': bool(r['confirmed'])}
                                          for r in rec]}
            if track:
                out['tracked'] = track_refined(acq, rec, whole, source, cfg)
        elif refine:
            out['refined'] = {'n_ms': 0, 'device_ms': 0.0, 'records': []}
            if track:
                out['tracked'] = {'device_ms': 0.0, 'chunks': 0, 'channels': []}
        acq.engine.close()
    return out


def weak_fix_report(assist, solver, fixes, cfg):
    """--weak-fix: per weak PRN the subframes decoded and the fixes it took part in (a fix is one
    (TOW, block) group of the solver's measurements; its time names it)."""
    import datetime
    from gpsmi import position as P
    stamps = {f[0] for f in fixes}
    groups = {}
    for r in solver.sat_results:
        groups.setdefault((r[1], r[7], r[6]), set()).add(r[0])
    took = {}
    for (tow, cyc, week), sats in groups.items():
        t = P.gps_datetime(tow, week) + datetime.timedelta(seconds=cyc * cfg.n_cyc / 1000)
        if len(sats) >= solver.min_sat and t.timestamp() in stamps:
            for s in sats:
                took[s] = took.get(s, 0) + 1
    return {'search_device_ms': round(assist.search_ms, 3),
            'channels': [{'prn': prn, 'bits': ch.n_bits, 'subframes': len(ch.frames), 'fixes': took.get(prn, 0)}
                         for prn, ch in assist.handoff.chan.items()]}


def load_ephemerides(path):
    """--ephemeris: {PRN: ephemeris} of a saved EPHEM_FILE (a JSON object keyed by the PRN)."""
    with open(path) as f:
        return {int(k): v for k, v in json.load(f).items()}


def save_ephemerides(path, ephs):
    """--save-ephemeris: {PRN: ephemeris} (position.EphemerisTable.ephem) as load_ephemerides reads
    it back: the subframe 1-3 parameters, numpy scalars as plain numbers."""
    from gpsmi import position as P
    keys = P.EPHEM_SF1 + P.EPHEM_SF2 + P.EPHEM_SF3
    out = {str(int(prn)): {k: getattr(e[k], 'tolist', lambda v=e[k]: v)() for k in keys}
           for prn, e in sorted(ephs.items())}
    with open(path, 'w') as f:
        json.dump(out, f)


def decoded_ephemerides(solver):
    """{PRN: ephemeris} of the satellites whose subframes 1-3 a PositionSolver has read."""
    return {s: o.data.ephem for s, o in solver.orbits.items() if o.data.ephem_ok}


def parse_time(text, ephs):
    """--time: GPS seconds of week, or a UTC timestamp turned into them with position.LEAPSEC and
    the week number of the ephemerides."""
    import datetime
    from gpsmi import position as P
    try:
        return float(text)
    except ValueError:
        pass
    t = datetime.datetime.fromisoformat(text.replace('Z', '+00:00'))
    if t.tzinfo is not None:
        t = t.astimezone(datetime.timezone.utc).replace(tzinfo=None)
    week = next(iter(ephs.values()))['weekNum'] + P.ROLLOVER * 1024
    start = datetime.datetime(1980, 1, 6) + datetime.timedelta(days=7 * week)
    return (t - start).total_seconds() + P.LEAPSEC


def snapshot(path, seconds, ephemerides, t_gps, near=None, start_stream=0, frontend=None, excise=False,
             blank=False, cancel=None, collective_km=None, spoof_k=None, antennas=(), beams=False, profile=False,
             array=False):
    """--snapshot: gpsmi.snapshot.snapshot_fix on the first `seconds` behind `start_stream`, read
    and filtered block by block as run() feeds its receiver.  `cancel`: --cancel's C/N0 threshold
    (snapshot.measure's `cancel`); None leaves everything as it is without the flag.
    `collective_km`: --collective's radius (snapshot_fix's collective=True within it); None: not asked for.
    `spoof_k`: --spoof-check's doubled PRNs that raise the alarm (snapshot_fix's spoof=True); None: not asked for.
    `antennas` (with `spoof_k`): the files of the further channels of a coherent recorder; every file gives one
    row of the snapshot, `path` the first, and the spoofing check names the authentic fix from the records'
    spatial signatures (snapshot_fix's antennas=A).
    `beams` (with `antennas`): --beams, every record is measured again on a beam of its own over the antennas, with
    a null at the spoofer where one is found (snapshot_fix's beams=True).
    `profile` (with `spoof_k`): --profile-check, every record's multi-tap correlation profile is tested for a second
    copy of the code within the guard of the peaks (snapshot_fix's profile=True).
    `array` (with one to three `antennas`, without `spoof_k`): --array-search, the satellites are searched for
    over all antennas at once and measured on their own beams (snapshot_fix's array=True); one
    further deep search of antenna 0 alone tells the report which of them that antenna would have found."""
    from gpsmi import ingest, pipeline, position as P, snapshot as S
    from gpsmi.acquisition import Acquisition
    from gpsmi.conditioning import Conditioner
    from gpsmi.engine import Config
    cfg = Config()
    need = int(round(seconds * 1000)) * cfg.code_samples
    with ingest.open_blocks(path, cfg, start_stream, frontend, antennas) as (source, raw_u8):
        cond, acq = Conditioner(cfg, raw_u8, excise, blank), None
        try:
            if antennas:                             # [A][NGPS] blocks, as they come (no conditioning stage is asked for)
                blocks, have = [], 0
                for blk in source:
                    blocks.append(np.array(blk))
                    have += blk.shape[1]
                    if have >= need:
                        break
            else:
                blocks, have = ingest.take(source, need, cond)
            if have < need:
                sys.exit(f'--snapshot: the recording holds {have} samples after stream {start_stream}, {seconds} s need {need}')
            acq = Acquisition(cfg, raw_u8=cond.out_raw_u8)
            t0 = time.perf_counter()
            stats = {}
            data = np.ascontiguousarray(np.concatenate(blocks, axis=1)[:, :need]) if antennas else np.concatenate(blocks)[:need]
            fix, meas, ms = S.snapshot_fix(acq, data, ephemerides, t_gps,
                                           pos=None if near is None else np.array(P.geo_to_ecef(*near)),
                                           cancel=cancel, stats=stats,
                                           **({} if spoof_k is None else {'spoof': True, 'min_doubled': spoof_k}),
                                           **({'antennas': 1 + len(antennas)} if antennas else {}),
                                           **({'beams': True} if beams else {}),
                                           **({'profile': True} if profile else {}),
                                           **({'array': True} if array else {}),
                                           **({} if collective_km is None else
                                              {'collective': True, 'collective_cfg': {'radius_m': 1.0e3 * collective_km}}))
            wall = time.perf_counter() - t0
            alone = None
            if array:                                # for the report only: what antenna 0 shows by itself
                freqs = [cfg.min_freq + cfg.step_freq * i
                         for i in range(int(round((cfg.max_freq - cfg.min_freq) / cfg.step_freq)))]
                alone = pipeline.largest_peak_hits(acq, np.ascontiguousarray(data[0]), sorted(ephemerides), freqs, 4,
                                                   need // cfg.code_samples // 4, corr_min=cfg.corr_min)
        finally:
            cond.close()
            if acq is not None:
                acq.engine.close()
    out = {'seconds': need / cfg.sample_rate, 'device_ms': round(ms, 3), 'wall_s': round(wall, 3),
           'measurements': [{'prn': int(m['prn']), 'sample': int(m['sample']), 'code_phase': round(float(m['code_phase']), 4),
                             'f_hz': round(float(m['f_hz']), 2),
                             'cn0_dbhz': None if np.isnan(m['cn0_dbhz']) else round(float(m['cn0_dbhz']), 2),
                             'source': m['source'].decode()} for m in meas],
           'ok': bool(fix.ok), 'reason': fix.reason, 'satellites': fix.prns, 'dropped': fix.dropped}
    if collective_km is not None:
        out['path'] = fix.path
        c = stats.get('collective')
        if c is not None:
            geo = P.ecef_to_geo(c['ecef'])
            out['collective'] = {'radius_km': collective_km, 'prns': c['prns'], 'margin': round(c['margin'], 2),
                                 'score': round(c['score'], 3), 'clock_lag': round(c['lag'], 3),
                                 'lat_deg': round(float(geo[0]), 6), 'lon_deg': round(float(geo[1]), 6),
                                 't_gps': round(c['t_gps'], 4), 'z': [round(float(v), 2) for v in c['z']],
                                 'level_ms': [round(float(v), 3) for v in c['level_ms']]}
    if spoof_k is not None:
        rep = fix.spoof if fix.spoof is not None else stats.get('spoof')
        sp = {'min_doubled': spoof_k, 'doubled': [] if rep is None else rep.doubled,
              'alarm': bool(rep is not None and rep.alarm), 'crowded': bool(rep is not None and rep.crowded),
              'separation_m': None if rep is None or rep.separation_m is None else round(rep.separation_m, 1),
              'fixes': []}
        for fx in (rep.fixes if rep is not None and rep.fixes else ()):
            if fx is None or not fx.ok:
                sp['fixes'].append(None if fx is None else {'ok': False, 'reason': fx.reason})
                continue
            geo = P.ecef_to_geo(fx.ecef)
            sp['fixes'].append({'ok': True, 'lat_deg': None if geo is None else round(float(geo[0]), 6),
                                'lon_deg': None if geo is None else round(float(geo[1]), 6),
                                'height_m': None if geo is None else round(float(geo[2]), 1),
                                'ecef_m': [round(float(v), 2) for v in fx.ecef], 'satellites': fx.prns,
                                'dropped': fx.dropped, 'residual_rms_m': round(fx.rms_m, 2)})
        if antennas:
            sp.update({'antennas': 1 + len(antennas), 'authentic': None if rep is None else rep.authentic,
                       'one_source': [False, False] if rep is None else [bool(v) for v in rep.one_source],
                       'one_direction': bool(rep is not None and rep.one_direction),
                       'signature_ms': round(float(stats.get('signature_ms', 0.0)), 3)})
        if profile:
            fits = [] if rep is None or rep.profile is None else rep.profile
            sp.update({'distorted': [] if rep is None else rep.distorted, 'profile_t_min': S.PROFILE_T_MIN,
                       'profile_ms': round(float(stats.get('profile_ms', 0.0)), 3),
                       'profile': [{'prn': f.prn, 'T': round(f.T, 2), 'snr1': round(f.snr1, 1), 'd1': round(f.d1, 3),
                                    'd2': round(f.d2, 3), 'rel_power': round(f.rel_power, 3), 'n_runs': f.n_runs}
                                   for f in fits]})
        out['spoof'] = sp
    if beams:
        before = stats.get('before_beams')
        out['beams'] = {'beams_ms': round(float(stats.get('beams_ms', 0.0)), 3),
                        'records': [{'prn': b['prn'], 'null': b['null'], 'confirmed': b['confirmed'],
                                     'gain_db': round(b['gain_db'], 2), 'flags': b['flags'],
                                     'cn0_before_dbhz': None if np.isnan(before['cn0_dbhz'][i])
                                     else round(float(before['cn0_dbhz'][i]), 2)}
                                    for i, b in enumerate(stats.get('beams', []))]}
    if array:
        out['array'] = {'antennas': 1 + len(antennas), 'array_ms': round(float(stats.get('array_ms', 0.0)), 3),
                        'signature_ms': round(float(stats.get('signature_ms', 0.0)), 3),
                        'beams_ms': round(float(stats.get('beams_ms', 0.0)), 3),
                        'hits': [{'prn': int(h[1]), 'norm_max_corr': round(float(h[0]), 2), 'f_hz': float(h[2]),
                                  'delay': int(h[3])} for h in stats.get('hits', [])],
                        'beams': [{'prn': b['prn'], 'confirmed': b['confirmed'], 'kept': b['kept'],
                                   'gain_db': round(b['gain_db'], 2), 'flags': b['flags']} for b in stats.get('beams', [])],
                        'antenna0_alone': sorted(int(h[1]) for h in alone)}
    if cancel is not None:
        out['cancelled'] = [{'prn': int(r['prn']), 'n_windows': int(r['n_windows']), 'n_skipped': int(r['n_skipped']),
                             'removed': round(float(r['energy_removed'] / r['energy_in']), 5) if r['energy_in'] > 0 else 0.0}
                            for r in stats.get('cancelled', [])]
    if fix.ok:
        geo = P.ecef_to_geo(fix.ecef)                # (None next to the Earth's centre)
        out['position'] = {'lat_deg': None if geo is None else round(float(geo[0]), 6),
                           'lon_deg': None if geo is None else round(float(geo[1]), 6),
                           'height_m': None if geo is None else round(float(geo[2]), 1),
                           'ecef_m': [round(float(v), 2) for v in fix.ecef]}
        out.update({'t_gps': round(fix.t_gps, 6), 'sample': fix.sample, 'g': round(fix.g, 3),
                    'residual_rms_m': round(fix.rms_m, 2),
                    'protect_m': None if not np.isfinite(fix.protect_m) else round(fix.protect_m, 1)})
    return {'file': os.path.basename(path), 'snapshot': out}


def print_snapshot(out):
    s = out['snapshot']
    print(f"{out['file']}: snapshot of {s['seconds']} s, {len(s['measurements'])} satellites measured "
          f"({s['device_ms']} ms on the device)")
    for r in s.get('cancelled', []):
        print(f"  cancelled PRN {r['prn']:2d}: {r['removed']:.4f} of the power in {r['n_windows']} code periods "
              f"({r['n_skipped']} skipped)")
    c = s.get('collective')
    if c is not None:
        print(f"  collective search within {c['radius_km']} km over PRNs {c['prns']}: peak {c['margin']} robust sigma above "
              f"the map at {c['lat_deg']:.6f} N {c['lon_deg']:.6f} E, GPS time {c['t_gps']} s, clock lag {c['clock_lag']}; "
              f"per satellite {c['z']}; levels {c['level_ms']} ms")
    sp = s.get('spoof')
    if sp is not None:
        print(f"  spoofing check: PRNs in the air twice {sp['doubled']}"
              f"{' (more than two copies of one: the two strongest kept)' if sp['crowded'] else ''}; "
              f"{'ALARM' if sp['alarm'] else 'no alarm'} (from {sp['min_doubled']} doubled PRNs on)")
        for name, fx in zip(('fix a', 'fix b'), sp['fixes']):
            if fx is not None and fx['ok']:
                print(f"  {name}: {fx['lat_deg']} N {fx['lon_deg']} E {fx['height_m']} m, {len(fx['satellites'])} satellites, "
                      f"residual rms {fx['residual_rms_m']} m")
            elif fx is not None:
                print(f"  {name}: no fix ({fx['reason']})")
        if sp['separation_m'] is not None:
            if sp.get('authentic') is not None:
                print(f"  the two fixes are {sp['separation_m']} m apart; the doubled signals of fix "
                      f"{'ab'[1 - sp['authentic']]} arrive from one direction over {sp['antennas']} antennas: "
                      f"fix {'ab'[sp['authentic']]} is authentic")
            elif 'antennas' in sp:
                print(f"  the two fixes are {sp['separation_m']} m apart; over {sp['antennas']} antennas "
                      f"{'both sets' if all(sp['one_source']) else 'neither set'} of doubled signals arrive from one "
                      f"direction: no verdict")
            else:
                print(f"  the two fixes are {sp['separation_m']} m apart; with one antenna which of them is authentic is "
                      f"not decided here")
        if 'antennas' in sp:
            print(f"  one direction for every signal over {sp['antennas']} antennas: {'YES' if sp['one_direction'] else 'no'}")
        if 'profile' in sp:
            print(f"  correlation profiles ({sp['profile_ms']} ms on the device), one per record; a second copy of the "
                  f"code shows from T {sp['profile_t_min']} on:")
            for f in sp['profile']:
                print(f"  profile PRN {f['prn']:2d}  T {f['T']:8.2f}  snr1 {f['snr1']:8.1f}  delays {f['d1']:+.3f} {f['d2']:+.3f}  "
                      f"second path {f['rel_power']:.3f} of the first  {'DISTORTED' if f['prn'] in sp['distorted'] else 'one path'}")
            print(f"  PRNs with a distorted profile {sp['distorted']}; doubled or distorted: "
                  f"{'ALARM' if sp['alarm'] else 'no alarm'}")
    ar = s.get('array')
    if ar is not None:
        print(f"  array search over {ar['antennas']} antennas ({ar['array_ms']} ms on the device; signatures "
              f"{ar['signature_ms']} ms, beams {ar['beams_ms']} ms): PRNs {[h['prn'] for h in ar['hits']]}; antenna 0 "
              f"alone would have found {ar['antenna0_alone']}")
        kept = {b['prn']: b for b in ar['beams']}
        for h in ar['hits']:
            b = kept.get(h['prn'])
            how = 'no beam' if b is None else f"beam gain {b['gain_db']:5.2f} dB  " + (
                'measured on the beam' if b['kept'] else 'not confirmed on the beam: dropped')
            print(f"  array PRN {h['prn']:2d}  normMaxCorr {h['norm_max_corr']:6.2f}  bin {h['f_hz']:+8.1f} Hz  "
                  f"delay {h['delay']:4d}  {how}")
    bm = s.get('beams')
    if bm is not None:
        print(f"  beams over the antennas ({bm['beams_ms']} ms on the device), one per record:")
        for b in bm['records']:
            was = 'n/a' if b['cn0_before_dbhz'] is None else f"{b['cn0_before_dbhz']:.1f}"
            print(f"  beam PRN {b['prn']:2d}  {'null at the spoofer' if b['null'] else 'no null':19s}  gain {b['gain_db']:5.2f} dB  "
                  f"flags {b['flags']}  cn0_dbhz on antenna 0 {was}  "
                  f"{'measured on the beam' if b['confirmed'] else 'not confirmed on the beam: antenna-0 values kept'}")
    for m in s['measurements']:
        cn0 = 'n/a' if m['cn0_dbhz'] is None else f"{m['cn0_dbhz']:.1f}"
        print(f"  PRN {m['prn']:2d}  sample {m['sample']:8d}  code_phase {m['code_phase']:9.4f}  f_hz {m['f_hz']:+9.2f}  "
              f"cn0_dbhz {cn0}  ({m['source']})")
    if s['ok']:
        p = s['position']
        where = f"ECEF {p['ecef_m']}" if p['lat_deg'] is None else \
            f"{p['lat_deg']:.6f} N {p['lon_deg']:.6f} E, height {p['height_m']:.1f} m"
        unseen = 'nothing bounds a bad measurement' if s['protect_m'] is None else \
            f"one bad measurement could move it {s['protect_m']} m unseen"
        print(f"fix from {len(s['satellites'])} satellites{' (dropped ' + str(s['dropped']) + ')' if s['dropped'] else ''}: "
              f"{where}; GPS time {s['t_gps']} s at sample {s['sample']}; geometry factor {s['g']}, "
              f"residual rms {s['residual_rms_m']} m; {unseen}")
    else:
        print(f"no snapshot fix: {s['reason']}")


def run(path, seconds=None, start_stream=0, save_pickle=None, ephemerides=None, cpu_acq=False, report_lag=16,
        excise=False, frontend=None, blank=False, deep_acq=None, refine=False, track=False, weak_fix=False,
        save_ephemeris=None, antennas=(), null=False, sweep=None, null_taps=1):
    """frontend: None (the recorder's u8 format at 2.048 Msps) or a dict of frontend.FrontEnd's
    keyword arguments (fs_in, fmt, if_hz, conjugate).  deep_acq: None, or the seconds of the
    recording's start that deep_acquisition searches for the PRNs the sweep did not acquire; refine:
    its hits are refined as well; track: the confirmed ones are tracked bit-synchronously.
    weak_fix (with deep_acq, refine and track): the receiver runs inside pipeline.WeakAssist, which
    searches the first deep_acq seconds behind the cold sweep, tracks what it confirms and merges
    those channels' subframes and code phases into the datagrams the solver is fed;
    the report gains 'weak_fix'.  save_ephemeris: a path for the ephemerides the run decoded.
    antennas: the files of the further channels of a coherent multi-antenna recorder, read in step
    with `path` (antenna 0, the reference element); null: null steering combines them ahead of
    everything else (pipeline.Receiver(antennas=A, null=True)) and the report gains
    'null': the flag (1 nulled, 0 passed through) and the predicted gain in dB of every block;
    null_taps: 1, or 3 / 5 / 7 space-time taps per antenna (nulling.NullSteer(taps=...)).
    sweep: None, True or a frame length: time-frequency excision (pipeline.Receiver(sweep=...),
    DESIGN.md 4.2m); the report gains 'sweep'."""
    from gpsmi import ingest, position as P
    from gpsmi.engine import Config
    from gpsmi.pipeline import Receiver, save_results
    cfg = Config()
    # (a recording: the datagrams may come out `report_lag` blocks behind the block they belong to, the
    # reader then runs ahead of the GPU instead of stalling it once a second -- pipeline.Receiver)
    with ingest.open_blocks(path, cfg, start_stream, frontend, antennas) as (source, raw_u8):
        array = dict(antennas=1 + len(antennas), null=True) if null else {}
        steer = None
        if null and null_taps > 1:                      # (a stage of the caller's: used by the chain, closed here)
            from gpsmi.nulling import NullSteer
            steer = NullSteer(cfg, antennas=1 + len(antennas), raw_u8=raw_u8, taps=null_taps)
            array['null'] = steer
        rx = Receiver(cfg, raw_u8=raw_u8, report_lag=report_lag, excise=excise, blank=blank, sweep=sweep, **array)
        null_flags, null_gain, sweep_counts = [], [], []
        if weak_fix:
            from gpsmi.pipeline import WeakAssist
            top = WeakAssist(rx, seconds=deep_acq)
        else:
            top = rx
        solver = P.PositionSolver(cfg.code_samples, cfg.n_cyc, ephemerides=ephemerides)
        max_blocks = None if seconds is None else int(seconds * 1000 // cfg.n_cyc)
        fixes, n_dg, n_blocks, found = [], 0, 0, None
        t0 = time.perf_counter()
        for raw in source:
            top.feed(raw)
            n_blocks += 1
            if null:
                null_flags.append(int(rx.nuller.last_flags[0]))
                null_gain.append(round(float(rx.nuller.last_gain_db[0]), 2))
            if sweep:
                sweep_counts.append(int(rx.sweeper.last_counts[0]))
            if found is None and not rx.sweep_all_freq:
                found = list(rx.found_sats)
            for dg in top.result_list[n_dg:]:          # (every datagram, in order: RESULT_LIST)
                n_dg += 1
                fixes += solver.feed(pickle.loads(dg))
            if max_blocks is not None and n_blocks >= max_blocks:
                break
        top.drain()
        for dg in top.result_list[n_dg:]:
            n_dg += 1
            fixes += solver.feed(pickle.loads(dg))
        wall = time.perf_counter() - t0
        if save_pickle:
            save_results(save_pickle, top.result_list)
        if save_ephemeris:
            save_ephemerides(save_ephemeris, decoded_ephemerides(solver))
        sats = sorted(rx.act_sat_set)
        if sweep:
            cells = 2 * rx.sweeper.n
            done = [c for c in sweep_counts if c >= 0]
            sweep_out = {'frame': rx.sweeper.frame, 'blocks_excised': sum(1 for c in done if c > 0),
                         'blocks_passed_through': len(sweep_counts) - len(done),
                         'mean_share': round(float(np.mean(done)) / cells, 4) if done else 0.0}
        weak = weak_fix_report(top, solver, fixes, cfg) if weak_fix else None
        rx.close()
        if steer is not None:
            steer.close()
    out = {'file': os.path.basename(path), 'blocks': n_blocks, 'signal_s': round(n_blocks * cfg.n_cyc / 1000.0, 3),
           'wall_s': round(wall, 3), 'x_realtime': round(n_blocks * cfg.n_cyc / 1000.0 / wall, 1) if wall else None,
           'acquired': [(int(s), float(f), int(d)) for _, s, f, d in (found or [])],
           'tracked': sats, 'datagrams': n_dg, 'fixes': len(fixes),
           'ephemerides_decoded': sorted(s for s, o in solver.orbits.items() if o.data.ephem_ok)}
    if fixes:
        xyz = np.array([f[1:] for f in fixes])
        late = xyz[len(xyz) // 2:]
        mean = late.mean(axis=0)
        lat, lon, alt = P.ecef_to_geo(mean)
        out['position'] = {'lat_deg': round(float(lat), 6), 'lon_deg': round(float(lon), 6),
                           'height_m': round(float(alt), 1), 'ecef_m': [round(float(v), 2) for v in mean],
                           'from': f'mean of the last {len(late)} fixes',
                           'sd_of_mean_m': round(float(np.linalg.norm(late.std(axis=0)) / np.sqrt(len(late))), 2)}
    if null:
        out['null'] = {'antennas': 1 + len(antennas), 'taps': max(1, null_taps), 'flags': null_flags,
                       'gain_db': null_gain,
                       'blocks_nulled': int(sum(null_flags))}
    if sweep:
        out['sweep'] = sweep_out
    if weak is not None:
        out['weak_fix'] = weak
    if cpu_acq:
        out['cpu_cold_acquisition'] = cpu_cold_acquisition(path)
    if deep_acq:
        out['deep_acquisition'] = deep_acquisition(path, deep_acq, start_stream,
                                                   {s for s, _, _ in out['acquired']}, frontend, refine=refine,
                                                   track=track)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('recording')
    ap.add_argument('--seconds', type=float, default=None, help='stop after this much signal')
    ap.add_argument('--start-stream', type=int, default=0, help='START_STREAM (gpsglob.py:16)')
    ap.add_argument('--save-pickle', default=None, help='write the datagram list as SAVE_PICKLE does')
    ap.add_argument('--ephemeris', default=None, help='a saved EPHEM_FILE (gpsEphem.json) to start from')
    ap.add_argument('--cpu-acq', action='store_true', help='time the CPU cold acquisition (configs[0]) too')
    ap.add_argument('--report-lag', type=int, default=16,
                    help='blocks a datagram may trail the block it belongs to (0: none, as a live receiver)')
    ap.add_argument('--excise', action='store_true',
                    help='remove narrowband interference (CW tones) from every block first (DESIGN.md 4.2b)')
    ap.add_argument('--blank', action='store_true',
                    help='zero pulsed / chirp interference in every block (after --excise, DESIGN.md 4.2d)')
    ap.add_argument('--sweep', type=int, nargs='?', const=True, default=None, metavar='L', choices=[32, 64, 128, 256],
                    help='remove swept / chirp interference in the time-frequency plane of frames of L samples '
                         '(default: tfexcision.default_frame, 64 at 2.048 Msps; after --excise, before --blank; '
                         'DESIGN.md 4.2m)')
    ap.add_argument('--format', default=None, choices=['c64', 'u8iq', 'sc8', 'sc16', 'r8'],
                    help='sample format of another front end (DESIGN.md 4.2c); default u8iq when --fs / --if is given')
    ap.add_argument('--fs', type=int, default=None, help='input sample rate in Hz (default 2048000)')
    ap.add_argument('--if', dest='if_hz', type=float, default=None,
                    help='IF of real input or tuner offset of complex input in Hz (sign: sideband)')
    ap.add_argument('--conjugate', action='store_true', help='mirror the spectrum of complex input')
    ap.add_argument('--deep-acq', type=float, default=None, metavar='SECONDS',
                    help='afterwards search the first SECONDS for the PRNs the sweep missed, code Doppler '
                         'compensated (DESIGN.md 4.2l); printed only')
    ap.add_argument('--refine', action='store_true',
                    help='with --deep-acq: refine its hits (fine Doppler, bit edge, code phase, C/N0; DESIGN.md 4.2f)')
    ap.add_argument('--track', action='store_true',
                    help='with --refine: track the confirmed hits bit-synchronously through the recording (DESIGN.md 4.2g)')
    ap.add_argument('--weak-fix', action='store_true',
                    help='with --track: merge the weak channels into the datagrams the position fix is made of (DESIGN.md 4.2h)')
    ap.add_argument('--save-ephemeris', default=None, metavar='PATH',
                    help='write the ephemerides the run decoded, in the format --ephemeris reads')
    ap.add_argument('--snapshot', type=float, default=None, metavar='SECONDS',
                    help='a fix from the first SECONDS alone, no decoded subframe (DESIGN.md 4.2i); needs --ephemeris and --time')
    ap.add_argument('--cancel', type=float, nargs='?', const=40.0, default=None, metavar='DBHZ',
                    help='with --snapshot: cancel the satellites measured at or above DBHZ (default 40) and measure '
                         'the others on what is left (DESIGN.md 4.2j)')
    ap.add_argument('--collective', type=float, nargs='?', const=15.0, default=None, metavar='RADIUS_KM',
                    help='with --snapshot and --near: when fewer than five satellites are measured, search position, '
                         'coarse time and clock collectively within RADIUS_KM (default 15) of --near (DESIGN.md 4.2k)')
    ap.add_argument('--spoof-check', type=int, nargs='?', const=2, default=None, metavar='K',
                    help='with --snapshot: look for PRNs that are in the air twice, raise the alarm from K of them on '
                         '(default 2) and solve both sets (DESIGN.md 4.2n); the exit status stays 0 either way')
    ap.add_argument('--profile-check', action='store_true',
                    help='with --snapshot --spoof-check: test every record\'s multi-tap correlation profile for a second '
                         'copy of the code within two chips, where the peaks see one; such PRNs count towards the alarm '
                         '(DESIGN.md 4.2r)')
    ap.add_argument('--time', default=None,
                    help='with --snapshot: time of the first sample read, GPS seconds of week or a UTC timestamp, within 30 s')
    ap.add_argument('--near', default=None, metavar='LAT,LON[,H]',
                    help='with --snapshot: the position as far as known (degrees, metres), within 50 km')
    ap.add_argument('--antenna', action='append', default=[], metavar='FILE',
                    help='the file of a further antenna of a coherent recorder, sample-aligned with the '
                         'recording (repeatable; the recording is antenna 0, the reference element)')
    ap.add_argument('--null', action='store_true',
                    help='null steering over the antennas against wideband jamming, ahead of everything '
                         'else (DESIGN.md 4.2l)')
    ap.add_argument('--null-taps', type=int, default=1, choices=(1, 3, 5, 7), metavar='T',
                    help='with --null: T = 3, 5 or 7 space-time taps per antenna instead of one weight, against '
                         'delay and filter mismatch between the channels and dense tone fields')
    ap.add_argument('--beams', action='store_true',
                    help='with --snapshot --spoof-check --antenna FILE ...: measure every record again on a beam of '
                         'its own over the antennas, with a null at the spoofer where one is found (DESIGN.md 4.2q)')
    ap.add_argument('--array-search', action='store_true',
                    help='with --snapshot --antenna FILE ... (one to three): search for the satellites over all antennas '
                         'at once and measure each on a beam of its own (DESIGN.md 4.2s)')
    ap.add_argument('--json', action='store_true', help='one JSON line instead of text')
    a = ap.parse_args()
    if a.refine and not a.deep_acq:
        ap.error('--refine needs --deep-acq SECONDS')
    if a.track and not a.refine:
        ap.error('--track needs --refine')
    if a.weak_fix and not a.track:
        ap.error('--weak-fix needs --track')
    frontend = None
    if a.format is not None or a.fs is not None or a.if_hz is not None or a.conjugate:
        frontend = {'fmt': a.format or 'u8iq', 'fs_in': a.fs or 2048000, 'if_hz': a.if_hz or 0.0,
                    'conjugate': a.conjugate}
    eph = load_ephemerides(a.ephemeris) if a.ephemeris else None
    if a.snapshot is not None:
        if not eph or a.time is None:
            ap.error('--snapshot needs --ephemeris and --time')
        if not 0.043 <= a.snapshot <= 8.0:            # (snapshot.min_samples: 86017 samples)
            ap.error('--snapshot SECONDS: 0.043 .. 8')
        near = None
        if a.near:
            near = [float(v) for v in a.near.split(',')]
            if len(near) not in (2, 3):
                ap.error('--near LAT,LON[,H]')
            near = (near + [0.0])[:3]
        if a.collective is not None and (near is None or not 0.1 <= a.collective <= 100.0):
            ap.error('--collective [RADIUS_KM]: needs --near, 0.1 .. 100 km')
        if a.spoof_check is not None and (a.spoof_check < 1 or a.cancel is not None or a.collective is not None):
            ap.error('--spoof-check [K]: K from 1 on, without --cancel / --collective')
        if a.array_search and (not 1 <= len(a.antenna) <= 3 or a.spoof_check is not None or a.cancel is not None
                               or a.collective is not None or a.beams):
            ap.error('--array-search: with one to three --antenna FILE, without --spoof-check / --cancel / --collective '
                     '/ --beams')
        if a.antenna and ((a.spoof_check is None and not a.array_search) or a.null or a.null_taps != 1 or frontend is not None or a.excise
                          or a.blank or len(a.antenna) > 7):
            ap.error('--antenna FILE with --snapshot: up to seven further channels, with --spoof-check or --array-search, in the '
                     'recorder\'s own format, without --null / --null-taps / --excise / --blank')
        if a.beams and not a.antenna:
            ap.error('--beams needs --antenna FILE ... (the beams combine the antennas)')
        if a.profile_check and a.spoof_check is None:
            ap.error('--profile-check needs --spoof-check (the profiles serve the spoofing check)')
        out = snapshot(a.recording, a.snapshot, eph, parse_time(a.time, eph), near, a.start_stream, frontend,
                       a.excise, a.blank, a.cancel, a.collective, a.spoof_check, a.antenna, a.beams, a.profile_check,
                       a.array_search)
        if a.json:
            print(json.dumps(out))
        else:
            print_snapshot(out)
        return
    if a.time is not None or a.near is not None:
        ap.error('--time / --near need --snapshot SECONDS')
    if a.beams:
        ap.error('--beams needs --snapshot SECONDS')
    if a.profile_check:
        ap.error('--profile-check needs --snapshot SECONDS')
    if a.array_search:
        ap.error('--array-search needs --snapshot SECONDS')
    if bool(a.antenna) != a.null:
        ap.error('--antenna FILE (the further channels) and --null go together')
    if a.null_taps != 1 and not a.null:
        ap.error('--null-taps needs --null')
    if a.antenna and (frontend is not None or a.deep_acq or a.cpu_acq):
        ap.error('--antenna: the recorder\'s own format, without --deep-acq / --cpu-acq')
    if a.cancel is not None:
        ap.error('--cancel needs --snapshot SECONDS')
    if a.collective is not None:
        ap.error('--collective needs --snapshot SECONDS')
    if a.spoof_check is not None:
        ap.error('--spoof-check needs --snapshot SECONDS')
    out = run(a.recording, a.seconds, a.start_stream, a.save_pickle, eph, a.cpu_acq, a.report_lag, a.excise,
              frontend, a.blank, a.deep_acq, a.refine, a.track, a.weak_fix, a.save_ephemeris, a.antenna, a.null,
              a.sweep, a.null_taps)
    if a.json:
        print(json.dumps(out))
        return
    print(f"{out['file']}: {out['blocks']} blocks = {out['signal_s']} s of signal in {out['wall_s']} s "
          f"({out['x_realtime']} x real time)")
    print(f"acquired {len(out['acquired'])} satellites: " + ', '.join(f'PRN {s} {f:+.0f} Hz' for s, f, _ in out['acquired']))
    print(f"tracked {out['tracked']}; {out['datagrams']} datagrams; ephemerides decoded for {out['ephemerides_decoded']}")
    if 'position' in out:
        p = out['position']
        print(f"{out['fixes']} fixes; {p['from']}: {p['lat_deg']:.6f} N {p['lon_deg']:.6f} E, height {p['height_m']:.1f} m "
              f"(SD of mean {p['sd_of_mean_m']} m)")
    else:
        print('no position fix (too little signal for subframes 1-3 of four satellites, or no ephemerides)')
    if 'sweep' in out:
        u = out['sweep']
        print(f"sweep excision, frames of {u['frame']}: {u['blocks_excised']} blocks excised, "
              f"{u['blocks_passed_through']} passed through, {100 * u['mean_share']:.1f} % of the plane removed")
    if 'null' in out:
        u = out['null']
        print(f"null steering over {u['antennas']} antennas: {u['blocks_nulled']} of {len(u['flags'])} blocks nulled")
        for b, (f, g) in enumerate(zip(u['flags'], u['gain_db'])):
            print(f"  block {b:4d}  flag {f}  gain {g:6.2f} dB")
    if 'weak_fix' in out:
        w = out['weak_fix']
        print(f"weak channels merged into the fix ({w['search_device_ms']} ms of search on the device): {len(w['channels'])}")
        for q in w['channels']:
            print(f"  PRN {q['prn']:2d}  bits {q['bits']:5d}  subframes decoded {q['subframes']}  fixes it took part in {q['fixes']}")
    if 'cpu_cold_acquisition' in out:
        c = out['cpu_cold_acquisition']
        print(f"CPU cold acquisition (configs[0], numpy path, {c['cores']} core): {c['wall_ms']} ms, {len(c['found'])} satellites")
    if 'deep_acquisition' in out:
        d = out['deep_acquisition']
        print(f"deep acquisition over {d['seconds']} s ({d['n_seg']} x {d['n_coh']} ms, {len(d['searched'])} PRNs, "
              f"{d['device_ms']} ms on the device): {len(d['found'])} more satellites")
        for s, f, dly, nmc in d['found']:
            print(f'  PRN {s:2d}  bin {f:+6.0f} Hz  delay {dly:4d}  normMaxCorr {nmc:.2f}')
        if 'refined' in d:
            r = d['refined']
            print(f"refined over {r['n_ms']} ms ({r['device_ms']} ms on the device):")
            for q in r['records']:
                cn0 = 'n/a' if q['cn0_dbhz'] is None else f"{q['cn0_dbhz']:.1f}"
                print(f"  PRN {q['prn']:2d}  f_hz {q['f_hz']:+9.2f}  edge_ms {q['edge_ms']:2d}  code_phase {q['code_phase']:8.3f}  "
                      f"cn0_dbhz {cn0}  ratio {q['ratio']:.2f}  confirmed {q['confirmed']}")
        if 'tracked' in d:
            t = d['tracked']
            print(f"tracked {len(t['channels'])} channels in {t['chunks']} chunks ({t['device_ms']} ms on the device):")
            for q in t['channels']:
                cn0 = 'n/a' if q['cn0_dbhz'] is None else f"{q['cn0_dbhz']:.1f}"
                print(f"  PRN {q['prn']:2d}  bits {q['bits']:5d}  f_hz {q['f_hz']:+9.2f}  code_phase {q['code_phase']:8.3f}  "
                      f"cn0_dbhz {cn0}  lock {q['lock']:+.2f}")


if __name__ == '__main__':
    main()
