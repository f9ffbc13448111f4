"""From the bit records of the bit-synchronous tracker (``gpsmi_wtrk_bit``) to
the hand-off the evaluation side reads: subframes with their sample times, one code phase per
32-ms block, and the ``(skippedData, frameLst, coPhLst)`` tuple ``position.PositionSolver.feed``
takes.  Host only, numpy; the decoder is ``navbits.eval_gps_bits``.

Clock.  Every position here -- ``tau`` of a record, ``ST`` of a frame, the stream number of a
code phase -- is counted on ONE sample clock, the one the tracker's ``first_sample`` was given
on.  Block ``s`` is the samples ``[s ngps, (s + 1) ngps)`` of that clock and is reported as
``streamNo = s``.  ``pipeline.Receiver`` stamps the first sample of the block it is fed with
``SMP_TIME`` AFTER adding the block's length (gpsrecv.py:471, "timestamp for data[0]"), so its
clock reads ``ngps`` at the first sample of the stream: a weak channel that is to share a
datagram with the receiver's own is opened and tracked on that clock
(``pipeline.WeakAssist``), and nothing is shifted here.

What ``position.OrbitTracker.eval_code_phase`` makes of the two numbers: ``ST % cs`` is the
integer code phase at the subframe's first bit and ``ST // cs`` counts its code period;
``coPh`` is where a code period starts, modulo ``cs``, in the middle of block ``streamNo``.
"""
import numpy as np

from . import navbits

L1_HZ = 1575.42e6


def code_period(f_hz, cs, f_offset=0.0, carrier_hz=L1_HZ):
    """Tc of gpsmi.h: the code period in samples at NCO frequency f_hz (float64, as written
    there)."""
    return cs / (1.0 + (np.asarray(f_hz, dtype=np.float64) - f_offset) / carrier_hz)


class WeakChannelNav:
    """What one weak channel's bit records add up to: ``frames`` (every subframe decoded, in
    order, ``'ST'`` set; ``frame_tau`` holds the unrounded positions) and ``co_ph`` (``(streamNo, coPh)`` of every block covered).  `cfg`
    gives code_samples and n_cyc; `f_offset` and `carrier_hz` are the tracker's."""

    def __init__(self, prn, cfg, f_offset=0.0, carrier_hz=L1_HZ):
        self.prn, self.cfg = int(prn), cfg
        self.f_offset, self.carrier_hz = float(f_offset), float(carrier_hz)
        self.frames, self.co_ph = [], []
        self.frame_tau = []                 # tau of each frame's first bit, unrounded
        self._ready = []                    # (end of the bit that completed it, frame)
        self._n_frames_out = self._n_co_out = 0
        self._next_bit_no = None
        self._open()

    def _open(self):
        z = np.zeros(0, np.float64)
        self._tau, self._tc, self._f, self._cn0, self._lock = z, z, z, z, z
        self._bits = np.zeros(0, np.int8)   # GPSBITS: the hard bits no subframe has taken yet
        self._pos = np.zeros(0, np.int64)   # ... and their indices into _tau
        self._blk = None                    # the next block to report

    @property
    def n_bits(self):
        return len(self._tau)

    @property
    def first_sample(self):
        """Where the first bit absorbed (since the last gap) starts; inf before any."""
        return float(self._tau[0]) if len(self._tau) else np.inf

    @property
    def covered_end(self):
        """Where the last bit absorbed ends; -inf before any."""
        return float(self._tau[-1] + 20.0 * self._tc[-1]) if len(self._tau) else -np.inf

    def absorb(self, records):
        """A run of this channel's WTRK_BIT_DTYPE records, in any chunking.  Zero records behind
        a channel's last bit of a call (GPSMI_WTRK_DATA_END) are ignored.  Returns the frames this
        call completed."""
        rec = np.ascontiguousarray(records)
        if rec.ndim != 1:
            raise ValueError('the records of one channel expected')
        if len(rec):
            live = rec.view(np.uint8).reshape(len(rec), -1).any(axis=1)
            if not live.all():
                rec = rec[:int(np.argmin(live))]
        if not len(rec):
            return []
        bit_no = rec['bit_no'].astype(np.int64)
        if (np.diff(bit_no) != 1).any():
            raise ValueError('bit_no must be consecutive within a call')
        if self._next_bit_no is not None and bit_no[0] != self._next_bit_no:
            self._open()                    # the channel was re-opened: nothing spans the gap
        self._next_bit_no = int(bit_no[-1]) + 1
        cs, ngps = self.cfg.code_samples, self.cfg.ngps
        n0 = len(self._tau)
        tau = rec['tau'].astype(np.float64)
        self._tau = np.concatenate([self._tau, tau])
        self._tc = np.concatenate([self._tc, code_period(rec['f_hz'], cs, self.f_offset, self.carrier_hz)])
        self._f = np.concatenate([self._f, rec['f_hz'].astype(np.float64)])
        self._cn0 = np.concatenate([self._cn0, rec['cn0_dbhz'].astype(np.float64)])
        self._lock = np.concatenate([self._lock, rec['lock'].astype(np.float64)])
        # hard bits and where they sit; the subframes are evalGpsBits' business, both polarities
        # and the restart behind a subframe that fails included
        self._bits = np.append(self._bits, np.where(rec['p_i'] >= 0, 1, -1).astype(np.int8))
        self._pos = np.append(self._pos, np.arange(n0, n0 + len(rec), dtype=np.int64))
        got, self._bits, self._pos = navbits.eval_gps_bits(self._bits, self._pos)
        for f in got:
            i = int(f['ST'])                # (the index went through in the place of the time)
            f['ST'] = int(np.rint(self._tau[i]))
            self.frames.append(f)
            self.frame_tau.append(float(self._tau[i]))
            self._ready.append((float(self._tau[i + 300] + 20.0 * self._tc[i + 300]), f))
        # one code phase per block that lies wholly inside tracked bits, measured mid-block
        if self._blk is None:
            self._blk = max(int(np.ceil(self._tau[0] / ngps)), self.co_ph[-1][0] + 1 if self.co_ph else 0)
        end = self.covered_end
        while (self._blk + 1) * ngps <= end:
            c = float(self._blk * ngps + ngps // 2)
            b = int(np.searchsorted(self._tau, c, side='right')) - 1
            k = min(max(int(np.floor((c - self._tau[b]) / self._tc[b])), 0), 19)
            self.co_ph.append((int(self._blk), float((self._tau[b] + k * self._tc[b]) % cs)))
            self._blk += 1
        return got

    def take(self, stream_no):
        """For the report at block `stream_no`: (frames completed by the end of that block, code
        phases up to it, the display values there), each handed out once.  None before the
        channel's first bit has ended."""
        edge = (stream_no + 1) * self.cfg.ngps
        ends = self._tau + 20.0 * self._tc
        i = int(np.searchsorted(ends, edge, side='right')) - 1
        if i < 0:
            return None
        n = self._n_frames_out
        while n < len(self._ready) and self._ready[n][0] <= edge:
            n += 1
        frames = [f for _, f in self._ready[self._n_frames_out:n]]
        self._n_frames_out = n
        m = self._n_co_out
        while m < len(self.co_ph) and self.co_ph[m][0] <= stream_no:
            m += 1
        cps = self.co_ph[self._n_co_out:m]
        self._n_co_out = m
        cn0 = float(self._cn0[i])
        show = {'AMP': 0.0 if np.isnan(cn0) else cn0, 'CRM': float(self._lock[i]), 'FRQ': float(self._f[i])}
        return frames, cps, show


class WeakHandoff:
    """The weak channels' side of the hand-off: absorb() the records as the tracker returns
    them, datagrams() hands out ``(streamNo, (0, frameLst, coPhLst))`` for every report block
    (``streamNo % NO_SEC == 0``, once a second, as the receiver's) that all open channels have
    tracked past.  What a datagram holds depends on the records alone, not on how they were
    chunked: a frame belongs to the first report block that ends at or behind the bit that
    completed it (the one after its 300), a code phase to the first at or behind its block.
    Frames carry 'SAT', 'AMP' (C/N0 in dB-Hz here), 'CRM' (the lock indicator), 'FRQ' and
    'SWP' as the receiver's do; a channel without a frame reports those alone."""

    def __init__(self, cfg, f_offset=0.0, carrier_hz=L1_HZ):
        self.cfg = cfg
        self.f_offset, self.carrier_hz = f_offset, carrier_hz
        self.no_sec = 1024 // cfg.n_cyc
        self.chan = {}
        self._next = None

    def open(self, prn):
        self.chan[int(prn)] = WeakChannelNav(prn, self.cfg, self.f_offset, self.carrier_hz)
        return self.chan[int(prn)]

    def close(self, prn):
        return self.chan.pop(int(prn), None)

    def absorb(self, prn, records):
        return self.chan[int(prn)].absorb(records)

    @property
    def next_report(self):
        """The first report block datagrams() has not finished; None before the first bit."""
        return self._next

    def datagrams(self):
        out, ngps = [], self.cfg.ngps
        while self.chan:
            if self._next is None:
                t0 = min(ch.first_sample for ch in self.chan.values())
                if not np.isfinite(t0):
                    break
                self._next = -(-int(t0 // ngps) // self.no_sec) * self.no_sec
            if any(ch.covered_end < (self._next + 1) * ngps for ch in self.chan.values()):
                break
            frame_lst, co_ph_lst = [], {}
            for prn, ch in self.chan.items():
                got = ch.take(self._next)
                if got is None:
                    continue
                frames, cps, show = got
                for f in [dict(f) for f in frames] or [{}]:
                    f['SAT'] = prn
                    f.update(show)
                    f['SWP'] = False
                    frame_lst.append(f)
                if cps:
                    co_ph_lst[prn] = cps
            if frame_lst:
                out.append((self._next, (0, frame_lst, co_ph_lst)))
            self._next += self.no_sec
        return out


def merge_datagrams(strong, weak):
    """One hand-off tuple from the receiver's (`strong`) and the weak channels' (`weak`), both
    unpickled, either may be None.  The strong entries stay the objects they are, in place; the
    weak PRNs follow; a PRN on both sides keeps its strong entries alone; skippedData is the
    strong one's."""
    if weak is None:
        return strong
    if strong is None:
        return weak
    skipped, frames, co_ph = strong
    have = set(co_ph) | {f['SAT'] for f in frames if 'SAT' in f}
    frames = list(frames) + [f for f in weak[1] if f.get('SAT') not in have]
    co_ph = dict(co_ph)
    for prn, lst in weak[2].items():
        if prn not in have:
            co_ph[prn] = lst
    return skipped, frames, co_ph


def report_stream(datagram, default=None):
    """The block a hand-off tuple was built at: the last stream number its code phases name."""
    last = [lst[-1][0] for lst in datagram[2].values() if lst]
    return int(max(last)) if last else default
