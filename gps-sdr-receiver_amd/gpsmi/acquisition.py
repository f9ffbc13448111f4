"""Host side of cold acquisition: the reference's ``sweepAllSats`` /
``findCodePhase`` / ``getNewSats`` interface (reference src/gpsrecv.py:217-274,
:423-440) over the GPU search surface.

The GPU computes every (Doppler bin, SV) cell of a call; the first-hit rule
(scan bins upward, the first bin over CORR_MIN claims the SV and removes it
from the list, gpsrecv.py:256-265) is applied here in the reference's order, so
the result list is the one the reference builds.
"""
import numpy as np

from . import _lib
from ._lib import REFINE_MAX_MS, REFINE_OUT_DTYPE, WTRK_STATE_DTYPE, check, ptr
from .engine import AcqEngine, Config

SAT_ALL = list(range(2, 33))          # gpsrecv.py:36
L1_HZ = 1575.42e6


def norm_max_corr(cell):
    """(peak - mean)/std of findCodePhase (gpsrecv.py:223) from a peak record,
    evaluated in float64 like the reference."""
    return (np.float64(cell['peak']) - np.float64(cell['mean'])) \
        / np.float64(cell['std'])


class Acquisition:
    """Drop-in for the module-level search functions of gpsrecv.py."""

    def __init__(self, cfg=None, engine=None, raw_u8=False):
        """raw_u8: `data` of the calls below is the recorder's uint16 (Q << 8 | I) block as
        streamData reads it (gpsrecv.py:162-173) instead of complex64; it is decoded on the GPU."""
        self.cfg = cfg or Config()
        self.engine = engine or AcqEngine(self.cfg)
        if raw_u8:
            self.engine.set_input_format(True)

    def bin_frequencies(self, freq, it_sweep):
        """Frequencies one sweepAllSats call visits (gpsrecv.py:248, :267-272),
        and the (sweepReady, next freq) it returns."""
        c = self.cfg
        freqs, ready, it = [], False, 0
        while freq < c.max_freq and it < it_sweep:
            freqs.append(freq)
            freq += c.step_freq
            if freq >= c.max_freq:
                ready = True
                freq -= c.max_freq - c.min_freq
            it += 1
        return freqs, ready, freq

    def sweepAllSats(self, data, freq, satLst, satFound, itSweep=2):
        """Same contract as gpsrecv.sweepAllSats (gpsrecv.py:241-274):
        ``satLst`` and ``satFound`` are mutated in place; returns
        ``(sweepReady, freq, sorted(satFound, reverse=True))`` with entries
        ``(normMaxCorr, satNo, freq, delay)``."""
        c = self.cfg
        avg = min(c.sweep_corr_avg, c.n_cyc)
        freqs, ready, freq_next = self.bin_frequencies(freq, itSweep)
        if freqs and satLst:
            prns = list(satLst)
            table = self.engine.search(data, prns, freqs, avg)
            for b, f in enumerate(freqs):
                hit = []
                for j, s in enumerate(prns):
                    if s not in satLst:
                        continue
                    nmc = norm_max_corr(table[b, j])
                    if nmc > c.corr_min:
                        satFound.append((nmc, s, f, int(table[b, j]['argmax'])))
                        hit.append(s)
                for s in hit:
                    satLst.remove(s)
        return ready, freq_next, sorted(satFound, reverse=True)

    def sweepWeakSats(self, data, freqs, satLst, satFound, n_coh=4, n_seg=25):
        """sweepAllSats's first-hit contract over the non-coherent surface
        (AcqEngine.search_noncoherent: mean |corr| of n_seg segments of n_coh ms each): the
        bins `freqs` are scanned in order, the first normMaxCorr > CORR_MIN claims an SV;
        ``satLst`` and ``satFound`` are mutated in place, entries are
        ``(normMaxCorr, satNo, freq, delay)`` with the code phase at the start of `data`;
        returns ``sorted(satFound, reverse=True)``.  `data` holds at least
        n_seg * n_coh code periods (several blocks of the stream, concatenated)."""
        c = self.cfg
        freqs = list(freqs)
        if freqs and satLst:
            prns = list(satLst)
            table = self.engine.search_noncoherent(data, prns, freqs, n_coh, n_seg)
            for b, f in enumerate(freqs):
                hit = []
                for j, s in enumerate(prns):
                    if s not in satLst:
                        continue
                    nmc = norm_max_corr(table[b, j])
                    if nmc > c.corr_min:
                        satFound.append((nmc, s, f, int(table[b, j]['argmax'])))
                        hit.append(s)
                for s in hit:
                    satLst.remove(s)
        return sorted(satFound, reverse=True)

    def sweepDeepSats(self, data, freqs, satLst, satFound, n_coh=4, n_seg=250, f_offset=0.0):
        """sweepWeakSats's first-hit contract over the deep surface (AcqEngine.search_deep: the
        non-coherent mean with every segment's magnitudes moved back by the code-Doppler slide
        of its bin, so that spans of seconds keep their peak): bins scanned in order, the first
        normMaxCorr > CORR_MIN claims an SV; ``satLst`` and ``satFound`` are mutated in place,
        entries are ``(normMaxCorr, satNo, freq, delay)`` with the code phase at the start of
        `data`; returns ``sorted(satFound, reverse=True)``.  `f_offset`: what the bin frequencies
        differ from the true Doppler by (a tuner's frequency error), 0 when they are Dopplers."""
        c = self.cfg
        freqs = list(freqs)
        if freqs and satLst:
            prns = list(satLst)
            table = self.engine.search_deep(data, prns, freqs, n_coh, n_seg, f_offset=f_offset)
            for b, f in enumerate(freqs):
                hit = []
                for j, s in enumerate(prns):
                    if s not in satLst:
                        continue
                    nmc = norm_max_corr(table[b, j])
                    if nmc > c.corr_min:
                        satFound.append((nmc, s, f, int(table[b, j]['argmax'])))
                        hit.append(s)
                for s in hit:
                    satLst.remove(s)
        return sorted(satFound, reverse=True)

    def sweepArraySats(self, data, antennas, freqs, satLst, satFound, n_coh=4, n_seg=250, f_offset=0.0):
        """sweepDeepSats's first-hit contract over the array surface (AcqEngine.search_array: the
        deep search over `antennas` = 2 .. 4 rows whose complex correlations are combined per lag,
        DESIGN.md 4.2s), for satellites that no single antenna shows.  `data`: [antennas][n] on
        the host or a (device pointer, n) pair with the rows n samples apart.  The same hit rule
        (bins scanned in order, the first normMaxCorr > CORR_MIN claims an SV) and the same hit
        format as sweepDeepSats; normMaxCorr is that of T, a power."""
        c = self.cfg
        freqs = list(freqs)
        if freqs and satLst:
            prns = list(satLst)
            table = self.engine.search_array(data, antennas, prns, freqs, n_coh, n_seg, f_offset=f_offset)
            for b, f in enumerate(freqs):
                hit = []
                for j, s in enumerate(prns):
                    if s not in satLst:
                        continue
                    nmc = norm_max_corr(table[b, j])
                    if nmc > c.corr_min:
                        satFound.append((nmc, s, f, int(table[b, j]['argmax'])))
                        hit.append(s)
                for s in hit:
                    satLst.remove(s)
        return sorted(satFound, reverse=True)

    def refineHits(self, data, found, n_ms=None, f_offset=0.0, **cfg):
        """Refines the ``(normMaxCorr, satNo, freq, delay)`` entries that sweepWeakSats /
        sweepDeepSats return (AcqEngine.refine: fine Doppler, bit edge, sub-sample code phase,
        C/N0 and a detection ratio of its own): one record per entry, in the same order.  `data`
        is the data the sweep searched; `n_ms` defaults to the largest multiple of 20 it holds
        (two code periods and the early / late spacing are kept in hand for the code slide)."""
        cs = self.cfg.code_samples
        n = data[1] if isinstance(data, tuple) else len(data)
        if n_ms is None:
            tap = cfg.get('tap_samples') or (1 if cs == 2048 else 8)
            n_ms = min((n - tap) // cs - 2, REFINE_MAX_MS) // 20 * 20
        hits = [(s, f, d) for _, s, f, d in found]
        return self.engine.refine(data, hits, n_ms, f_offset=f_offset, **cfg)

    def trackHits(self, data, refined, n_bits=None, data_start=0, first_sample=0, refine_tap=0,
                  f_offset=0.0, **cfg):
        """Opens a bit-synchronous tracking channel on every record of refineHits
        (open_weak_channels; `data_start` is the stream index of the first sample of the data they
        were refined on) and tracks it through `data`, whose first sample has stream index
        `first_sample` (AcqEngine.track_weak).  `n_bits` defaults to what `data`
        can hold.  Returns (records, states); go on with engine.track_weak(next_data, states, ...,
        first_sample=...) for the chunks that follow."""
        states = open_weak_channels(refined, self.cfg, data_start, refine_tap, f_offset=f_offset)
        n = data[1] if isinstance(data, tuple) else len(data)
        if n_bits is None:
            n_bits = max(1, n // (20 * self.cfg.code_samples))
        return self.engine.track_weak(data, states, n_bits, first_sample=first_sample,
                                      f_offset=f_offset, **cfg)

    def cancelHits(self, data, rec, f_offset=0.0, out=None):
        """Takes the satellites of `rec` out of `data` (AcqEngine.cancel): records
        of refineHits (code_phase is the code start at the first sample) or snapshot.MEAS_DTYPE
        records (a code start lies at sample + code_phase), the strongest (cn0_dbhz) first.
        `data` and `out` as in AcqEngine.cancel.  Returns (out, records CANCEL_OUT_DTYPE in the
        order cancelled)."""
        rec = np.atleast_1d(np.asarray(rec))
        order = np.argsort(-np.nan_to_num(rec['cn0_dbhz'].astype(np.float64), nan=-np.inf), kind='stable')
        return self.engine.cancel(data, signature_sats(rec[order]), out=out, f_offset=f_offset)

    def signatureHits(self, data, rec, antennas, f_offset=0.0, **cfg):
        """The spatial signatures of the records `rec` over `antennas` coherent channels
        (AcqEngine.signatures): records of refineHits (code_phase is the code start
        at the first sample) or snapshot.MEAS_DTYPE records (a code start lies at sample +
        code_phase), in the order given; a PRN may appear more than once.  `data`: [antennas][n] on
        the host or a (device pointer, n) pair with the rows n samples apart.
        Returns (cov complex128 [R][A][A], n_win)."""
        return self.engine.signatures(data, signature_sats(rec), antennas, f_offset=f_offset, **cfg)[:2]

    def profileHits(self, data, rec, f_offset=0.0, **cfg):
        """The multi-tap correlation profiles of the records `rec` (AcqEngine.profiles; DESIGN.md
        4.2r): snapshot.MEAS_DTYPE records or records of refineHits (profile_sats: the runs start
        at the record's bit edge), in the order given; a PRN may appear more than once.  `data`: one
        row of samples on the host or a (device pointer, n) pair; `cfg`: half_taps, coh_ms, n_runs, carrier_hz.
        Returns (cov complex128 [R][K][K], n_runs)."""
        sats = profile_sats(rec, self.cfg.code_samples, cfg.get('half_taps', 0), f_offset,
                            cfg.get('carrier_hz', L1_HZ))
        return self.engine.profiles(data, sats, f_offset=f_offset, **cfg)[:2]

    def deepRows(self, data, prns, freqs, n_coh=4, n_seg=250, f_offset=0.0):
        """The deep surface kept whole (AcqEngine.search_deep with rows): the
        table of sweepDeepSats' search and a DeviceBuffer of float32 [len(prns)][len(freqs)]
        [code_samples] with the surface of every cell, for AcqEngine.collective.  The caller
        frees the buffer.  -> (table, rows)."""
        from .engine import DeviceBuffer
        prns, freqs = list(prns), list(freqs)
        rows = DeviceBuffer(len(prns) * len(freqs) * self.cfg.code_samples * 4, self.cfg.device)
        try:
            table = self.engine.search_deep(data, prns, freqs, n_coh, n_seg, f_offset=f_offset, rows=rows)
        except Exception:
            rows.free()
            raise
        return table, rows

    def search_table(self, data, prns, freqs, n_avg):
        """The whole surface, no pruning (BASELINE configs 2 and 4)."""
        return self.engine.search(data, prns, freqs, n_avg)


def code_starts(rec):
    """tau float64 [R] of records of refineHits (code_phase is the code start at the first sample) or
    snapshot.MEAS_DTYPE (a code start lies at sample + code_phase).  Host only."""
    rec = np.atleast_1d(np.asarray(rec))
    start = rec['sample'].astype(np.float64) if 'sample' in rec.dtype.names else 0.0
    return start + rec['code_phase'].astype(np.float64)


def signature_sats(rec):
    """(prn, f_hz, tau) of records of refineHits or snapshot.MEAS_DTYPE, tau as code_starts gives
    it, in the order given.  Host only."""
    rec = np.atleast_1d(np.asarray(rec))
    return [(int(r['prn']), float(r['f_hz']), float(t)) for r, t in zip(rec, code_starts(rec))]


def profile_sats(rec, cs, half_taps=0, f_offset=0.0, carrier_hz=L1_HZ):
    """(prn, skip_ms, f_hz, tau) of snapshot.MEAS_DTYPE records (a code start lies at sample +
    code_phase, a bit starts at `edge`) or of records of refineHits (code start code_phase, a bit
    starts edge_ms periods on), in the order given.  skip_ms counts the windows of
    gpsmi_acq_profile -- the first is the first code start with half_taps samples ahead of it --
    up to the first one that starts a bit; 0 where the record names no edge.  Host only."""
    rec = np.atleast_1d(np.asarray(rec))
    Lh = int(half_taps) or (8 if cs == 2048 else 32)
    meas = 'sample' in rec.dtype.names
    out = []
    for r, tau in zip(rec, code_starts(rec).tolist()):
        f = float(r['f_hz'])
        Tc = cs / (1.0 + (f - f_offset) / carrier_hz)
        edge = float(r['edge']) if meas else tau + float(r['edge_ms']) * Tc if r['edge_ms'] >= 0 else np.nan
        k = int(np.floor((Lh - tau) / Tc))
        while np.rint(tau + float(k) * Tc) >= Lh:
            k -= 1
        while np.rint(tau + float(k) * Tc) < Lh:
            k += 1
        skip = (int(np.rint((edge - tau) / Tc)) - k) % 20 if np.isfinite(edge) else 0
        out.append((int(r['prn']), skip, f, tau))
    return out


def hit_at(rec, sample, cfg, carrier_hz=L1_HZ):
    """What ``initInst`` needs to open a channel on a refined hit (a record of refineHits) at a
    later sample index of the stream the hit was refined on: ``(freq, delay)`` with the refined
    Doppler and the code phase moved by the code slide -f / carrier_hz samples per sample,
    modulo ``code_samples`` and rounded to a whole sample as findCodePhase delivers delays.
    Host only.  `sample` counts from the first sample of the refined data."""
    cs = cfg.code_samples
    if rec['code_phase'] < 0:
        raise ValueError('the record has no code phase (its prompt tap was not the largest)')
    f = float(rec['f_hz'])
    phase = float(rec['code_phase']) - f / carrier_hz * float(sample)
    return f, int(np.rint(phase)) % cs


def open_weak_channels(refined, cfg, data_start=0, refine_tap=0, carrier_hz=L1_HZ, f_offset=0.0):
    """Fresh tracking states (WTRK_STATE_DTYPE) for records of refineHits: gpsmi_wtrk_open per
    record -- tau = data_start + code_phase + edge_ms code periods, f_hz the refined Doppler,
    theta 0.  Host only.  `data_start`: the stream index of the first sample of the refined data;
    `refine_tap`: the tap_samples refinement ran with (0: its default)."""
    lib = _lib.load()
    rec = np.ascontiguousarray(np.array(refined, dtype=REFINE_OUT_DTYPE, ndmin=1))
    out = np.zeros(len(rec), WTRK_STATE_DTYPE)
    for i in range(len(rec)):
        check(lib.gpsmi_wtrk_open(ptr(rec[i:i + 1]), cfg.code_samples, int(refine_tap), int(data_start),
                                  float(carrier_hz), float(f_offset), ptr(out[i:i + 1])), 'gpsmi_wtrk_open')
    return out


def weak_bits(records):
    """Hard decisions on the bit records of one channel or of several ([..., n_bits],
    WTRK_BIT_DTYPE): ``(bits, transitions)``, bits = sign Re P_b as +-1 (valid up to one global
    sign, and only under phase lock), transitions[b - 1] = sign Re(P_b conj(P_{b-1})) as +-1
    (-1: the data bit changed), which needs frequency lock alone.  Host only."""
    p = records['p_i'].astype(np.float64) + 1j * records['p_q'].astype(np.float64)
    bits = np.where(p.real >= 0, 1, -1).astype(np.int8)
    d = (p[..., 1:] * np.conj(p[..., :-1])).real
    return bits, np.where(d >= 0, 1, -1).astype(np.int8)


def getNewSats(actSatSet, foundSats, cpQLst, max_sat=11):
    """gpsrecv.getNewSats (gpsrecv.py:423-440): keep satellites whose channels
    still correlate, fill up to MAX_SAT with the strongest new ones."""
    good = {s for s, (q, l) in cpQLst.items() if q > 0 or l > 0}
    fs = [e for e in foundSats if e[1] not in good]
    found = good | {e[1] for e in fs[:max_sat - len(good)]}
    common = actSatSet & found
    return actSatSet - common, found - common
