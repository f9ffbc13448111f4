"""The receiver's block loop and its hand-off to the evaluation process.

Mirror of the data path of ``gpsrecv.processData`` (reference
src/gpsrecv.py:445-548) without its asyncio / socket plumbing: feed it the
32-ms blocks in order, it runs the cold sweep, selects satellites, tracks them
and returns, whenever the reference would send one, the hand-off datagram
``pickle.dumps((skippedData, frameLst, coPhLst))`` (gpsrecv.py:496-519).
``Receiver.command(b'SWEEP')`` / ``b'STOP'`` are the two commands the
evaluation side can send back (gpsrecv.py:522-536).  ``send_udp`` and
``save_results`` are the reference's two sinks (gpsrecv.py:513-517, :205-212).
"""
import pickle
import socket

import numpy as np

from . import _lib, receiver as R
from .acquisition import SAT_ALL, Acquisition, getNewSats
from .engine import Config

UDP_IP = '127.0.0.1'            # gpsglob.py:79
UDP_PORT = 61431                # gpsglob.py:82


class Receiver:
    def __init__(self, cfg=None, sat_all=None, raw_u8=False, report_lag=0, excise=None, blank=None,
                 antennas=1, null=None, sweep=None):
        """raw_u8: feed() takes the recorder's uint16 (Q << 8 | I) blocks exactly as streamData
        reads them from the file (gpsrecv.py:162-173); the decode to complex64 happens inside
        the GPU kernels, every datagram is byte-identical to the complex64 path's.
        report_lag = L: feed() returns a datagram L blocks after the block the reference sends it
        on (0, the default: on that block) -- the once-a-second host work then runs while the GPU
        has L newer blocks queued instead of idling through it; the datagrams are the same.
        excise = True or an excision.Excision: feed() first removes narrowband interference from
        each block on the GPU into a page-locked complex64 block, which then takes the complex64
        path unchanged (with raw_u8 the excision decodes, the engines run in complex64).  None, the
        default: no excision, everything as without the argument.
        blank = True or a blanking.PulseBlanker: the same for pulsed and swept interference (pulse
        blanking).  With both, each block is excised, then blanked, on the device (one copy in, one
        out): a tone raises every sample's power and would hide the pulses from the blanker, while
        the pulses only add a flat level to the excision's spectrum.  The PulseBlanker then takes
        complex64 (raw_u8=False).  None, the default: no blanking.
        antennas = A > 1 with null = True or a nulling.NullSteer: feed() takes [A][NGPS], the blocks
        of A coherent antennas, and null steering (power inversion, antenna 0 the reference) combines
        them into one complex64 block ahead of the other stages.  The defaults (1, None): one antenna,
        everything as without the arguments.
        sweep = True or a tfexcision.SweepExcision: time-frequency excision against swept and chirp
        interference, between the excision and the blanking.  None, the default: off, everything as
        without the argument.  The chain is `conditioner` (conditioning.Conditioner);
        its `last` is the block the engines saw."""
        from .conditioning import Conditioner
        self.cfg = cfg or Config()
        self.conditioner = Conditioner(self.cfg, raw_u8, excise, blank, null, antennas, sweep)
        self.excision, self.blanker = self.conditioner.excision, self.conditioner.blanker
        self.nuller, self.sweeper = self.conditioner.nuller, self.conditioner.sweeper
        self.raw_u8 = self.conditioner.out_raw_u8     # (the engines see the filters' complex64)
        self.sat_all = list(SAT_ALL if sat_all is None else sat_all)
        self.acq = Acquisition(self.cfg, raw_u8=self.raw_u8)
        self.pool, self.pool_no, self.pool_worker = R.initMultiProcPool(self.cfg.max_sat,
                                                                        self.cfg, self.raw_u8)
        self.pool.report_lag = int(report_lag)
        self.running = True
        self.smp_time = np.int64(0)                  # SMP_TIME, gpsrecv.py:29
        self.act_sat_set = set()
        self.co_ph_lst, self.cp_q_lst = {}, {}
        self.skipped_data = 0
        self.result_list = []                        # RESULT_LIST (SAVE_PICKLE)
        self._start_sweep()

    def _start_sweep(self, first=True):              # gpsrecv.py:450-451, :462-463, :529-533
        self.sweep_all_freq = True
        if first:
            self.doppler_freq = self.cfg.min_freq    # a SWEEP command keeps the current bin
        self.sat_lst = self.sat_all.copy()
        self.found_sats = []

    def command(self, msg):
        """b'SWEEP' restarts the cold search, b'STOP' ends the run."""
        if msg == b'SWEEP':
            self.drain()                             # (cpQLst must be current for getNewSats)
            self._start_sweep(first=False)
        elif msg == b'STOP':
            self.running = False

    def feed(self, data, skip=0):
        """One block (complex64[NGPS], or uint16[NGPS] when raw_u8; [antennas][NGPS] with null
        steering); `skip` = streams lost before it
        (gpsrecv.py:469-471).  Returns the pickled hand-off or None."""
        c = self.cfg
        # (one page-locked block serves every call: the acquisition reads it before it returns,
        # the tracking pool copies it into its own input ring)
        data = self.conditioner.apply(data)
        self.skipped_data += skip * c.ngps
        self.smp_time += (1 + skip) * c.ngps
        if self.sweep_all_freq:
            ready, self.doppler_freq, self.found_sats = self.acq.sweepAllSats(
                data, self.doppler_freq, self.sat_lst, self.found_sats,
                itSweep=c.it_sweep_all)
            if ready:
                self.sweep_all_freq = False
                dele, new = getNewSats(self.act_sat_set, self.found_sats, self.cp_q_lst,
                                       c.max_sat)
                if dele:
                    self.pool_worker, self.act_sat_set = R.delPoolStreams(
                        self.pool, self.pool_no, self.pool_worker, self.act_sat_set, dele)
                self.pool_worker, self.act_sat_set = R.initPoolStreams(
                    self.pool, self.pool_no, self.pool_worker, self.act_sat_set, new,
                    self.found_sats)
            return None
        if not self.act_sat_set:                     # (nothing acquired: the reference's satCalc
            return None                              # returns [], no datagram)
        # the block is enqueued on the GPU; the host catches up once a second, at the block
        # the reference sends its datagram on (R.satCalcLazy)
        res = None
        for batch in R.satCalcLazy(self.act_sat_set, self.pool, self.pool_worker, data,
                                   self.smp_time):
            res = self.hand_off(batch) or res
        return res

    def drain(self):
        """Absorb the blocks that are still on their way (before anything that reads the
        channel state from outside: a command, close, a test)."""
        self.pool.absorb_pending()
        for batch in self.pool.take_done():
            self.hand_off(batch)

    def hand_off(self, batch):
        """gpsrecv.py:496-519 for the K blocks of a batch, the last of which carries the
        frames: every block appends (streamNo, coPh) for the channels that correlated -- a
        satellite enters coPhLst at its first such block, in the order satCalc returned the
        results -- and when any frame exists (once a second) the datagram is built and the
        accumulators are reset."""
        ngps = self.cfg.ngps
        cp = batch.code_phase                        # [K][satellites in actSatSet order]
        good = cp >= 0
        stream_nos = [t // ngps for t in batch.smp_times]       # (np.int64, as SMP_TIME//NGPS is there)
        n_good = good.sum(axis=0)
        first = np.where(n_good > 0, good.argmax(axis=0), len(stream_nos))
        cols = cp.T.tolist()
        for col in np.argsort(first, kind='stable').tolist():
            if n_good[col] == 0:
                break
            lst = self.co_ph_lst.setdefault(batch.sats[col], [])
            if n_good[col] == len(stream_nos):
                lst.extend(zip(stream_nos, cols[col]))
            else:
                lst.extend((stream_nos[k], cols[col][k]) for k in np.flatnonzero(good[:, col]).tolist())
        frame_lst = []
        for sw_fq, sat_no, f_lst, co_ph, cp_q in batch.res:
            frame_lst += f_lst
            self.cp_q_lst[sat_no] = cp_q
        if not frame_lst:
            return None
        res = pickle.dumps((self.skipped_data, frame_lst, self.co_ph_lst))
        self.result_list.append(res)
        self.co_ph_lst = {}
        self.skipped_data = 0
        return res

    def close(self):
        self.drain()
        R.closeMultiProcPool(self.pool)
        self.acq.engine.close()
        self.conditioner.close()


def send_udp(sock, res, ip=UDP_IP, port=UDP_PORT):
    """gpsrecv.py:513-517"""
    sock.sendto(res, (ip, port))


def save_results(path, result_list):
    """saveResults (gpsrecv.py:205-212): the list of datagrams as one pickle,
    the file LOAD_PICKLE replays in gpseval."""
    with open(path, 'wb') as f:
        pickle.dump(result_list, f)


def make_udp_socket():
    return socket.socket(socket.AF_INET, socket.SOCK_DGRAM)


def largest_peak_hits(acq, data, prns, freqs, n_coh=4, n_seg=250, f_offset=0.0, corr_min=None):
    """Deep-search hits ``(normMaxCorr, satNo, freq, delay)`` of satellites known to be there, one
    per PRN at the bin of its largest peak.  (sweepDeepSats' first bin over the threshold is a
    sidelobe for a strong satellite, and its own sidelobes raise the std normMaxCorr divides by.)
    `corr_min`: for satellites that may be absent or weak -- only the bins whose normMaxCorr
    exceeds it compete, and a PRN without such a bin has no hit.  (Beside strong satellites the
    largest peak of a weak PRN is a strong one's cross-correlation in another bin, on a surface
    those raise as a whole: a peak normMaxCorr does not take for a detection.)"""
    tab = acq.engine.search_deep(data, list(prns), list(freqs), n_coh, n_seg, f_offset=f_offset)
    nmc = (tab['peak'].astype(np.float64) - tab['mean']) / tab['std']
    if corr_min is None:
        best = tab['peak'].argmax(axis=0)
        return [(float(nmc[b, j]), s, freqs[b], int(tab[b, j]['argmax'])) for j, (s, b) in enumerate(zip(prns, best))]
    over = nmc > corr_min
    best = np.where(over, tab['peak'], -np.inf).argmax(axis=0)
    return [(float(nmc[b, j]), s, freqs[b], int(tab[b, j]['argmax']))
            for j, (s, b) in enumerate(zip(prns, best)) if over[b, j]]


def array_peak_hits(acq, data, antennas, prns, freqs, n_coh=4, n_seg=250, f_offset=0.0, corr_min=None):
    """largest_peak_hits over the array surface (AcqEngine.search_array over `antennas` rows,
    DESIGN.md 4.2s): hits ``(normMaxCorr, satNo, freq, delay)``, one per PRN at the bin of its
    largest peak, with `corr_min` only among the bins whose normMaxCorr exceeds it.  `data`:
    [antennas][n] on the host or a (device pointer, n) pair with the rows n samples apart."""
    tab = acq.engine.search_array(data, antennas, list(prns), list(freqs), n_coh, n_seg, f_offset=f_offset)
    nmc = (tab['peak'].astype(np.float64) - tab['mean']) / tab['std']
    over = nmc > corr_min if corr_min is not None else np.ones(nmc.shape, bool)
    best = np.where(over, tab['peak'], -np.inf).argmax(axis=0)
    return [(float(nmc[b, j]), s, freqs[b], int(tab[b, j]['argmax']))
            for j, (s, b) in enumerate(zip(prns, best)) if over[b, j]]


def hits_of_picks(picks, cols, prns, freqs, corr_min):
    """The hits ``(z, satNo, freq, lag)`` of AcqEngine.peaks' picks [nsv][k] and columns
    [nsv][k][2][nbins]: one per pick with z > corr_min, in pick order.  The bin is
    not the pick's own (the bin of largest z lies beside a strong or doubled satellite, whose own
    peaks raise the std of its bin) but largest_peak_hits' choice on the pick's column: among the
    bins with z > corr_min at that lag the one of largest S, the first of equal ones."""
    hits = []
    for j, s in enumerate(prns):
        for pk, col in zip(picks[j], cols[j]):
            if pk['lag'] < 0 or not pk['z'] > corr_min:
                continue
            over = col[1] > corr_min
            b = int(np.where(over, col[0], -np.inf).argmax())
            hits.append((float(pk['z']), s, freqs[b], int(pk['lag'])))
    return hits


def peak_candidates(acq, data, prns, freqs, n_coh, n_seg, f_offset=0.0, corr_min=None, k=4, stats=None):
    """Up to `k` deep-search hits ``(z, satNo, freq, lag)`` per PRN, more than two chips apart in
    code phase: one deep search that keeps its surfaces (Acquisition.deepRows), then
    AcqEngine.peaks over them and hits_of_picks (`corr_min` defaults to the configuration's).  A
    PRN that is in the air twice yields two hits where largest_peak_hits keeps the stronger.
    `stats`: a dict that receives picks, cols and the device ms of the two calls."""
    prns, freqs = list(prns), list(freqs)
    corr_min = acq.cfg.corr_min if corr_min is None else corr_min
    _, rows = acq.deepRows(data, prns, freqs, n_coh, n_seg, f_offset=f_offset)
    try:
        search_ms = acq.engine.last_ms()
        picks, cols = acq.engine.peaks(rows, len(prns), len(freqs), k=k)
        peaks_ms = acq.engine.last_ms()
    finally:
        rows.free()
    if stats is not None:
        stats.update(picks=picks, cols=cols, search_ms=search_ms, peaks_ms=peaks_ms)
    return hits_of_picks(picks, cols, prns, freqs, corr_min)


def refine_centred(acq, data, found, f_offset=0.0, **cfg):
    """Acquisition.refineHits, and again for every confirmed hit that came back without a code
    phase because its early or late tap was larger than its prompt: the search's integer delay
    was one off (the peak of a second's search lies where the sliding code spent most of it), so
    the hit is refined one tap spacing towards the larger tap, twice at the most.  `cfg`:
    refineHits' keywords (df_half, ...).  -> (found with the delays used, records, device ms)."""
    cs = acq.cfg.code_samples
    tap = 1 if cs == 2048 else 8
    found = list(found)
    rec = acq.refineHits(data, found, f_offset=f_offset, **cfg)
    ms = acq.engine.last_ms()
    for _ in range(2):
        bad = [i for i, r in enumerate(rec) if r['confirmed'] == 1 and r['code_phase'] < 0]
        if not bad:
            break
        for i in bad:
            nmc, s, f, d = found[i]
            e, _, l = rec[i]['tap_metric']
            found[i] = (nmc, s, f, int(d + (-tap if e > l else tap)) % cs)
        rec[bad] = acq.refineHits(data, [found[i] for i in bad], f_offset=f_offset, **cfg)
        ms += acq.engine.last_ms()
    return found, rec, ms


GHOST_HZ, GHOST_DB = 5.0, 10.0


def ghosts_of(strong, refined, hz=GHOST_HZ, db=GHOST_DB):
    """Which records of `refined` are the satellite of the refinement record `strong` seen through
    another PRN's code: within `hz` of it modulo the code's 1-kHz line spacing
    and not reading within `db` of it (a record without a C/N0 does not).  A `strong` that is not
    confirmed or has no C/N0 has no ghosts.  -> bool per record."""
    if strong['confirmed'] != 1 or np.isnan(strong['cn0_dbhz']):
        return np.zeros(len(refined), bool)
    d = np.abs((refined['f_hz'] - strong['f_hz'] + 500.0) % 1000.0 - 500.0)
    return (d <= hz) & ~(refined['cn0_dbhz'] > strong['cn0_dbhz'] - db)


class WeakTracker:
    """Weak channels (states of acquisition.open_weak_channels) followed through a stream in
    chunks: push() the samples that follow those pushed so far and get every channel's new bit
    records (AcqEngine.track_weak).  Between chunks the samples before the
    earliest channel's next bit are dropped and first_sample moves up; the records are the same
    bytes for any chunking.  `first_sample`: the stream index of the first sample pushed, on the
    clock the states were opened on.  `track_cfg`: track_weak's keyword arguments."""

    def __init__(self, engine, states, first_sample=0, **track_cfg):
        self.engine, self.states, self.cfg = engine, states, track_cfg
        self.first = int(first_sample)
        cs = engine.cfg.code_samples
        self.tap = track_cfg.get('tap_samples') or (1 if cs == 2048 else 8)
        self.pending = None
        self.device_ms, self.chunks = 0.0, 0

    def push(self, data):
        """-> [records of channel h that this chunk added] in the order of `states`."""
        self.pending = data if self.pending is None else np.concatenate([self.pending, data])
        if not len(self.states):
            return []
        n_bits = len(self.pending) // (20 * self.engine.cfg.code_samples) + 1
        bits, new = self.engine.track_weak(self.pending, self.states, n_bits, first_sample=self.first,
                                           **self.cfg)
        self.device_ms += self.engine.last_ms()
        self.chunks += 1
        out = [bits[h, :int(new['bit_no'][h] - self.states['bit_no'][h])] for h in range(len(new))]
        self.states = new
        self._trim()
        return out

    def _trim(self):
        lo = int(np.floor(self.states['tau']).min()) - self.tap if len(self.states) else self.first + len(self.pending)
        if lo > self.first:
            self.pending = self.pending[lo - self.first:]
            self.first = lo

    def drop(self, h):
        self.states = np.delete(self.states, h)
        if self.pending is not None:
            self._trim()


class WeakAssist:
    """A Receiver with the satellites its 4-ms sweep cannot acquire added to its datagrams
    (DESIGN.md 4.2h).  feed() forwards every block to the receiver.  The first `seconds` of blocks
    after the receiver's cold sweep has finished are kept; on them the receiver's own Acquisition
    runs the deep search (sweepDeepSats, `n_coh`-ms segments) for the PRNs the receiver does not
    track, refines the hits (refineHits) and opens a bit-synchronous channel on every confirmed one
    (`min_snr`: and of at least that C/N0 in dB-Hz), on the receiver's sample clock.  From then on
    the channels are tracked every `chunk_blocks` blocks (WeakTracker; `track_cfg` goes to
    track_weak), their bits decoded and their code phases reported block by block
    (weaknav.WeakHandoff), and each datagram of the receiver leaves merged with the weak channels'
    of the same report block (weaknav.merge_datagrams) -- which the weak side has only once it has
    tracked past that block, so a merged datagram trails the receiver's by up to `chunk_blocks`
    blocks.  Without a weak channel every datagram is returned as the receiver made it, bytes
    and block.  A PRN the receiver acquires itself is closed here; a lost stretch of the stream
    (`skip`) closes all of them and the search starts over."""

    def __init__(self, receiver, seconds=1.0, n_coh=4, min_snr=None, chunk_blocks=16, **track_cfg):
        from .weaknav import WeakHandoff
        self.rx, self.cfg = receiver, receiver.cfg
        self.n_coh, self.min_snr, self.chunk_blocks = int(n_coh), min_snr, int(chunk_blocks)
        self.n_seg = int(round(seconds * 1000)) // self.n_coh
        if not 1 <= self.n_seg <= 32768 or self.chunk_blocks < 1:
            raise ValueError('seconds / n_coh / chunk_blocks out of range')
        self.track_cfg = track_cfg
        self.handoff = WeakHandoff(self.cfg, track_cfg.get('f_offset', 0.0),
                                   track_cfg.get('carrier_hz', 1575.42e6))
        self.result_list = []                        # every datagram handed out, in order
        self.found, self.refined = [], None          # what the deep search and refinement returned
        self.own_refined = None                      # ... and the receiver's own satellites, refined alike
        self.search_ms = 0.0
        self._n_rx = len(receiver.result_list)
        self._out, self._last_s = [], -1
        self._rearm()

    def _rearm(self):
        for prn in list(self.handoff.chan):
            self.handoff.close(prn)
        self.tracker = None
        self.searched = False
        self._kept, self._kept_start, self._n_kept = [], None, 0
        self._blocks = []                            # fed since the tracker's last chunk
        self._strong, self._weak = [], {}

    @property
    def weak_prns(self):
        return list(self.handoff.chan)

    def feed(self, block, skip=0):
        """Receiver.feed's arguments; returns a pickled hand-off (the receiver's, the weak
        channels', or both merged) or None."""
        rx = self.rx
        sweeping = rx.sweep_all_freq
        rx.feed(block, skip)
        if skip:
            self._flush()
            self._rearm()
        self._strong += rx.result_list[self._n_rx:]
        self._n_rx = len(rx.result_list)
        block = rx.conditioner.last                  # (what the engines saw)
        if self.tracker is None:
            if not self.searched and not sweeping and not rx.sweep_all_freq:
                self._keep(block)
        else:
            self._close_taken()
            self._blocks.append(np.array(block))
            if len(self._blocks) >= self.chunk_blocks:
                self._track([np.concatenate(self._blocks)])
        self._release()
        return self._hand_out()

    def _hand_out(self):
        if not self._out:
            return None
        res = self._out.pop(0)
        self.result_list.append(res)
        return res

    def _keep(self, block):
        if self._kept_start is None:
            self._kept_start = int(self.rx.smp_time)     # the receiver's clock at block[0]
        self._kept.append(np.array(block))
        self._n_kept += len(block)
        if self._n_kept >= max(self.n_seg * self.n_coh, 43) * self.cfg.code_samples:
            self._search()

    def _search(self):
        from .acquisition import open_weak_channels
        c, acq = self.cfg, self.rx.acq
        whole = np.concatenate(self._kept)
        self._kept, self.searched = [], True
        freqs = [c.min_freq + c.step_freq * i for i in range(int(round((c.max_freq - c.min_freq) / c.step_freq)))]
        sat_lst = [s for s in self.rx.sat_all if s not in self.rx.act_sat_set]
        f_off = self.track_cfg.get('f_offset', 0.0)
        self.found = acq.sweepDeepSats(whole[:self.n_seg * self.n_coh * c.code_samples], freqs, sat_lst, [],
                                       n_coh=self.n_coh, n_seg=self.n_seg, f_offset=f_off)
        self.search_ms = acq.engine.last_ms()
        if not self.found:
            return
        self.found, self.refined, ms = refine_centred(acq, whole, self.found, f_offset=f_off)
        self.search_ms += ms
        good = (self.refined['confirmed'] == 1) & (self.refined['code_phase'] >= 0)
        good &= ~self._ghosts(whole, freqs, f_off)
        if self.min_snr is not None:
            good &= self.refined['cn0_dbhz'] >= self.min_snr     # (NaN: no)
        rec = self.refined[good]
        if not len(rec):
            return
        states = open_weak_channels(rec, c, data_start=self._kept_start, f_offset=f_off)
        for prn in states['prn']:
            self.handoff.open(prn)
        self.tracker = WeakTracker(acq.engine, states, self._kept_start, **self.track_cfg)
        step = self.chunk_blocks * c.ngps
        self._track([whole[i:i + step] for i in range(0, len(whole), step)])

    GHOST_HZ, GHOST_DB = GHOST_HZ, GHOST_DB

    def _ghosts(self, whole, freqs, f_off):
        """Which refined hits are the receiver's own satellites seen through another PRN's code:
        the C/A codes' cross-correlation (-24 dB, -21 dB at the worst Doppler offset) turns a
        satellite 20 dB above the search's sensitivity into a peak the search finds, at the strong
        satellite's Doppler plus a multiple of the code's 1-kHz line spacing, and such a channel
        would track it and decode the STRONG satellite's subframes under the wrong PRN.  The
        receiver's satellites go through the same search (largest_peak_hits) and the same
        refinement; a hit within GHOST_HZ of one of them modulo 1 kHz that reads GHOST_DB or more
        below it is dropped.  -> bool per refined record."""
        c, acq = self.cfg, self.rx.acq
        own = sorted(self.rx.act_sat_set)
        self.own_refined = None
        out = np.zeros(len(self.refined), bool)
        if not own:
            return out
        hits = largest_peak_hits(acq, whole[:self.n_seg * self.n_coh * c.code_samples], own, freqs, self.n_coh,
                                 self.n_seg, f_offset=f_off)
        self.search_ms += acq.engine.last_ms()
        _, self.own_refined, ms = refine_centred(acq, whole, hits, f_offset=f_off)
        self.search_ms += ms
        for o in self.own_refined:
            out |= ghosts_of(o, self.refined, self.GHOST_HZ, self.GHOST_DB)
        return out

    def _track(self, chunks):
        self._blocks = []
        for data in chunks:
            before = self.tracker.states['bit_no'].copy()
            new = self.tracker.push(data)
            st = self.tracker.states
            for h in range(len(st) - 1, -1, -1):
                self.handoff.absorb(st['prn'][h], new[h])
                if st['bit_no'][h] == before[h] and not st['flags'][h] & _lib.WTRK_DATA_END:
                    self._close(h)               # (a state that is no longer finite stops for good)
        for s, dg in self.handoff.datagrams():
            if s > self._last_s:                 # (the receiver's of that block has left already)
                self._weak[s] = dg

    def _close(self, h):
        self.handoff.close(self.tracker.states['prn'][h])
        self.tracker.drop(h)

    def _close_taken(self):
        st = self.tracker.states
        for h in range(len(st) - 1, -1, -1):
            if int(st['prn'][h]) in self.rx.act_sat_set:
                self._close(h)

    def _release(self, everything=False):
        """Moves to _out what can leave: the receiver's datagrams as they are while no weak channel
        is open; else those of report blocks the weak side has finished (all, with `everything`),
        merged with its datagram of that block."""
        from .weaknav import merge_datagrams, report_stream
        live = self.tracker is not None and len(self.tracker.states) > 0 and not everything
        if not live and not self._weak:
            if self._strong:
                self._last_s = report_stream(pickle.loads(self._strong[-1]), self._last_s)
            self._out += self._strong
            self._strong = []
            return
        done = self.handoff.next_report          # the weak side is complete below this block
        while self._strong:
            tup = pickle.loads(self._strong[0])
            s = report_stream(tup, int(self.rx.smp_time) // self.cfg.ngps)
            if live and (done is None or s >= done):
                break
            dg = self._strong.pop(0)
            for w in sorted(k for k in self._weak if k < s):       # (the receiver had none there)
                self._out.append(pickle.dumps(self._weak.pop(w)))
            self._last_s = s
            weak = self._weak.pop(s, None)
            self._out.append(dg if weak is None else pickle.dumps(merge_datagrams(tup, weak)))
        if not self._strong and (not live or not self.rx.act_sat_set):
            for w in sorted(self._weak):
                self._out.append(pickle.dumps(self._weak.pop(w)))

    def _flush(self):
        self.rx.drain()
        self._strong += self.rx.result_list[self._n_rx:]
        self._n_rx = len(self.rx.result_list)
        if self.tracker is not None and self._blocks:
            self._track([np.concatenate(self._blocks)])
        self._release(everything=True)

    def drain(self):
        """Everything still on its way, on either side; the datagrams go to result_list."""
        self._flush()
        while self._out:
            self._hand_out()

    def close(self):
        self.drain()
        self.rx.close()
