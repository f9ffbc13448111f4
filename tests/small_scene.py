"""A small synthetic scene for the option and shape cases of refinement (gpsmi_acq_refine) and weak
tracking (gpsmi_acq_track), plain numpy, and the case tables test_acq_refine.py / test_acq_track.py
(CPU: the restatements' margins and guards) and test_gpu_refine_cases.py / test_gpu_track_cases.py
(GPU against the restatements) share.

render(): complex Gaussian noise of sigma 0.35 (as synth: 0.35 / sqrt 2 per component) plus, per
satellite (prn, doppler f, delay, amp),
    amp * replica[floor(pos) mod cs] * bit * exp(2 pi j f i / fs),   pos = (i - delay) (1 + (f - f_offset) / carrier)
with random data bits, one per 20 code periods, the bit edge `edge` periods after the code start at
`delay`.  The replica is held over a sample (no interpolation), so replica[0] first appears at
sample ceil(delay): that is the delay a hit carries.  Amplitudes 0.02 at 2048 and 0.01 at 16368 are
38 / 41 dB-Hz by amp^2 fs / sigma^2; a millisecond then holds 8 / 11 dB, so 40 ms decide.

Every restatement is computed once per process (lru_cache) and handed out unchanged."""
import functools
import math

import numpy as np

from deep_ref import L1_HZ
from ifx_ref import quantise
from refine_ref import refine_ref
import wtrk_ref as W

SIGMA = 0.35
AMP = {2048: 0.02, 16368: 0.01}
L2_HZ = 1.2276e9


def _tone(f, fs, n, blk=4096):
    """exp(2 pi j f i / fs), i < n, as the product of a coarse and a fine table (both exact to an
    ulp: the phases are reduced mod 1 in float64 first)."""
    a = np.arange((n + blk - 1) // blk, dtype=np.float64) * blk
    r = np.arange(blk, dtype=np.float64)
    t = np.exp(2j * np.pi * np.mod(f * a / fs, 1.0))[:, None] * np.exp(2j * np.pi * np.mod(f * r / fs, 1.0))[None, :]
    return t.ravel()[:n]


@functools.lru_cache(maxsize=4)
def render(cs, n, sats, seed, f_offset=0.0, carrier=L1_HZ, edge=0):
    """-> complex128 [n]; sats: a tuple of (prn, doppler, delay, amp)."""
    from gpsmi import codes
    rng = np.random.default_rng(seed)
    x = (SIGMA / np.sqrt(2.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    i = np.arange(n, dtype=np.float64)
    fs = 1000.0 * cs
    for prn, f, delay, amp in sats:
        rep = codes.code_replica(int(prn), cs)
        fl = np.floor((i - delay) * (1.0 + (f - f_offset) / carrier))
        j = np.mod(fl, cs)
        period = (fl - j) / cs                                    # exact
        bits = 1.0 - 2.0 * rng.integers(0, 2, size=n // (20 * cs) + 4)
        bit_no = np.floor((period - edge) / 20.0).astype(np.int64) + 2
        x += (amp * rep[j.astype(np.int64)] * bits[bit_no]) * _tone(f, fs, n)
    x.setflags(write=False)
    return x


def renderings(x):
    """-> (complex64, the recorder's u16 (Q << 8 | I), the complex64 the raw-u8 engine decodes)."""
    from gpsmi.synth import raw_to_c64
    c64 = x.astype(np.complex64)
    raw = quantise(x)
    dec = raw_to_c64(raw)
    for a in (c64, raw, dec):
        a.setflags(write=False)
    return c64, raw, dec


def hit_of(sat, f_hit=None, early=0):
    prn, f, delay, _ = sat
    return (prn, float(round(f / 100.0) * 100.0 if f_hit is None else f_hit), int(math.ceil(delay)) - early)


# ---- refinement --------------------------------------------------------------------------------------

def _sats(cs, which=(0, 1)):
    k = cs / 2048.0
    base = [(6, -3210.0, 412.3), (15, 2470.0, 1650.7), (23, 4230.0, 957.4), (29, -1810.0, 1311.6),
            (10, 30.0, 705.2), (2, 3590.0, 120.8), (19, -2390.0, 1888.5), (31, 790.0, 1502.1)]
    return [(p, f, round(d * k, 1), AMP[cs]) for p, f, d in (base[w] for w in which)]


class RefineCase:
    """One call of gpsmi_acq_refine: the scene, the hits and the options."""

    def __init__(self, name, cs, n_ms, seed, sats=None, hits=None, raw=False, gap=1e-3, zeros=False,
                 **opts):
        self.name, self.cs, self.n_ms, self.seed, self.raw, self.gap = name, cs, n_ms, seed, raw, gap
        self.zeros = zeros
        self.opts = opts                               # df_step, df_half, tap, f_offset, carrier_hz
        self.sats = _sats(cs) if sats is None else sats
        self.hits = [hit_of(s) for s in self.sats] if hits is None else hits
        self.tap = opts.get('tap') or (1 if cs == 2048 else 8)
        self.n = (n_ms + 2) * cs + self.tap
        self.edge = 7

    def __repr__(self):
        return self.name

    def data(self):
        return _refine_data(self)

    def ref(self, decoded=False):
        """refine_ref of the complex64 rendering, or of what the raw-u8 engine decodes."""
        return _refine_ref(self, decoded)

    def engine_kw(self):
        o = self.opts
        return dict(df_step=o.get('df_step', 2.0), df_half=o.get('df_half', 120.0),
                    tap_samples=o.get('tap', 0), f_offset=o.get('f_offset', 0.0),
                    carrier_hz=o.get('carrier_hz', L1_HZ))


@functools.lru_cache(maxsize=None)
def _refine_data(c):
    if c.zeros:
        x = np.zeros(c.n, np.complex128)
    else:
        x = render(c.cs, c.n, tuple(c.sats), c.seed, c.opts.get('f_offset', 0.0),
                   c.opts.get('carrier_hz', L1_HZ), c.edge)
    return renderings(x)


@functools.lru_cache(maxsize=None)
def _refine_ref(c, decoded):
    c64, _, dec = c.data()
    with np.errstate(invalid='ignore', divide='ignore'):
        return refine_ref(dec if decoded else c64, c.hits, c.n_ms, c.cs, **c.opts)


def _tap_sats():
    s = _sats(2048, (0, 1, 2, 3))
    return [(p, f, float(d), a) for (p, f, _, a), d in zip(s, (0, 511, 512, 2047))]


def _many():
    sats = _sats(2048, range(8))
    return sats, [hit_of(s, round(s[1] / 100.0) * 100.0 - 70.0 + 20.0 * v) for s in sats for v in range(8)]


def _build_refine_cases():
    c = []
    one = lambda cs: _sats(cs, (0,))
    for cs in (2048, 16368):
        c.append(RefineCase('min-%d' % cs, cs, 40, 101, raw=True))
    c += [RefineCase('tail-60', 2048, 60, 202), RefineCase('tail-100', 2048, 100, 103)]
    c += [RefineCase('lanes-1300', 2048, 1300, 104, raw=True), RefineCase('lanes-1320', 2048, 1320, 105, raw=True)]
    c += [RefineCase('threads-5140', 2048, 5140, 106, sats=one(2048)),
          RefineCase('threads-5160', 2048, 5160, 107, sats=one(2048)),
          RefineCase('max-8000', 2048, 8000, 108, sats=one(2048))]
    # n_df 1, 3, 3, 1024; the hits sit on the truth so that the peak can be interior.  At steps of
    # 1 and 0.5 Hz neighbouring rows differ by (pi 0.02)^2 / 3 (2 delta - step) step of the peak at
    # most (the 20-ms sinc^2 around its top: 1.3e-3 and 3.3e-4), so no seed reaches a gap of 1e-3
    # with the peak inside; the gap asserted there is 2e-4, twice the cap on the grid's deviation
    # (1e-4), which is what an equal argmax needs.
    on = [hit_of(s, s[1]) for s in _sats(2048)]
    for i, (step, half, gap) in enumerate(((1.0, 0.4, 1e-3), (1.0, 1.0, 2e-4), (2.0, 2.0, 1e-3),
                                           (0.5, 255.75, 2e-4))):
        c.append(RefineCase('n_df-%g-%g' % (step, half), 2048, 100, (110, 111, 312, 1113)[i], hits=on, gap=gap,
                            df_step=step, df_half=half))
    for name, off, seed in (('rows-first', +60.0, 115), ('rows-last', -60.0, 116)):
        c.append(RefineCase(name, 2048, 100, seed, hits=[hit_of(s, s[1] + off) for s in _sats(2048)],
                            df_step=5.0, df_half=20.0))
    c.append(RefineCase('tap-512', 2048, 60, 617, sats=_tap_sats(), raw=True, tap=512))
    c += [RefineCase('tap-1-16368', 16368, 40, 218, raw=True, tap=1),
          RefineCase('tap-4092-16368', 16368, 40, 119, raw=True, tap=4092)]
    for cs, seeds in ((2048, (220, 421)), (16368, (120, 121))):
        c += [RefineCase('slide-minus-%d' % cs, cs, 60, seeds[0], raw=True, f_offset=-3e6),
              RefineCase('slide-plus-%d' % cs, cs, 60, seeds[1], raw=True, f_offset=3e6)]
    c.append(RefineCase('slide-plus-L2-2048', 2048, 60, 222, raw=True, f_offset=3e6, carrier_hz=L2_HZ))
    sats, hits = _many()
    c.append(RefineCase('many-64', 2048, 40, 3823, sats=sats, hits=hits))
    c.append(RefineCase('misaligned', 2048, 100, 124, hits=[hit_of(s, early=1) for s in _sats(2048)]))
    c.append(RefineCase('zeros', 2048, 40, 0, zeros=True, raw=True))
    return c


REFINE_CASES = _build_refine_cases()
RATIO_BAND = (2.25, 2.75)                         # min_ratio 2.5 +- 0.25
TAP_GAP = 1e-3


def refine_margins(ref, grid, gap):
    """The distance of every decision of a restatement from its threshold; -> (ok, text)."""
    ok, lines = True, []
    for h in range(len(ref)):
        r = ref[h]
        top = np.sort(grid[h].ravel())[-2:]
        g = (top[1] - top[0]) / top[1]
        tm = r['tap_metric']
        t = min(abs(tm[0] - tm[1]), abs(tm[2] - tm[1])) / tm[1]
        good = not (RATIO_BAND[0] <= r['ratio'] <= RATIO_BAND[1]) and g > gap and t > TAP_GAP
        ok = ok and good
        lines.append('hit %2d prn %2d ratio %7.3f  top-two gap %.2e  tap gap %.2e%s'
                     % (h, r['prn'], r['ratio'], g, t, '' if good else '   <-- marginal'))
    return ok, '\n'.join(lines)


# ---- weak tracking -------------------------------------------------------------------------------------

OPEN_MS = 100
TRACK_SPARE_MS = 24                               # the edge (up to 20 periods) and the last windows


class TrackCase:
    """One scene of gpsmi_acq_track: channels opened by open_ref from refine_ref on the first
    OPEN_MS milliseconds of the same data."""

    def __init__(self, name, cs, n_bits, seed, sats=None, absent=None, chans=None, **opts):
        self.name, self.cs, self.n_bits, self.seed, self.opts = name, cs, n_bits, seed, opts
        self.sats = _sats(cs) if sats is None else sats
        self.absent = absent                           # (prn, freq, delay) of a PRN not in the scene
        self.chans = chans                             # None: one channel per satellite; else per
        self.n = (max(20 * n_bits, OPEN_MS) + TRACK_SPARE_MS) * cs      # channel (satellite, df)
        self.edge = 7

    def __repr__(self):
        return self.name

    def scene_kw(self):
        return dict(f_offset=self.opts.get('f_offset', 0.0), carrier_hz=self.opts.get('carrier_hz', L1_HZ))

    def data(self):
        return _track_data(self)

    def states(self):
        """The opened channels (dicts of wtrk_ref)."""
        return _track_states(self)

    def ref(self, n_bits=None, n=None, first_sample=0):
        """track_ref over the first n samples of the complex64 rendering, taken to lie first_sample
        down the stream (every state's tau moved with it)."""
        return _track_ref(self, self.n_bits if n_bits is None else n_bits, n, first_sample)


@functools.lru_cache(maxsize=None)
def _track_data(c):
    kw = c.scene_kw()
    return renderings(render(c.cs, c.n, tuple(c.sats), c.seed, kw['f_offset'], kw['carrier_hz'], c.edge))


@functools.lru_cache(maxsize=None)
def _track_states(c):
    c64 = c.data()[0]
    kw = c.scene_kw()
    hits = [hit_of(s) for s in c.sats] + ([c.absent] if c.absent else [])
    rec, _, _ = refine_ref(c64[:(OPEN_MS + 2) * c.cs + 8], hits, OPEN_MS, c.cs, **kw)
    states = []
    for r, hit in zip(rec, hits):
        if r['code_phase'] < 0:                        # (no vertex: an absent candidate, or a code
            r = r.copy()                               # that slides samples within a millisecond;
            r['code_phase'] = float(hit[2]) + 0.25     # a quarter sample keeps tau off the integers)
            r['tap_metric'] = (0.0, 1.0, 0.0)
        states.append(W.open_ref(r, c.cs, **kw))
    if c.chans is not None:
        out = []
        for s, df in c.chans:
            st = dict(states[s], mu_ring=list(states[s]['mu_ring']))
            st['f_hz'] = st['f_acc'] = st['f_hz'] + df
            out.append(st)
        states = out
    return states


@functools.lru_cache(maxsize=None)
def _track_ref(c, n_bits, n, first_sample):
    c64 = c.data()[0]
    n = len(c64) if n is None else n
    states = c.states()
    if first_sample:                                   # the same scene further down the stream
        states = [dict(s, tau=s['tau'] + first_sample) for s in states]
    return W.track_ref(c64[:n], states, n_bits, c.cs, first_sample=first_sample, **c.opts)


FAR = 2 ** 31 + 4096
MANY_DF = (-3.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5)


def _build_track_cases():
    c = [TrackCase('ring', 2048, 60, 401, absent=(3, 1000.0, 100))]
    for i, o in enumerate((dict(pll_bw=8.0, fll_bw=2.0, dll_bw=1.0, pull_in_bits=3), dict(pll_bw=-1.0),
                           dict(fll_bw=-1.0, pull_in_bits=-1), dict(dll_bw=2.0))):
        c.append(TrackCase('options-%d' % i, 2048, 30, 202, **o))
    c += [TrackCase('taps-1', 16368, 6, 203, tap=1), TrackCase('taps-15', 16368, 6, 203, tap=15)]
    for cs in (2048, 16368):
        c += [TrackCase('slide-minus-%d' % cs, cs, 10, 204, f_offset=-3e6),
              TrackCase('slide-plus-%d' % cs, cs, 10, 205, f_offset=3e6)]
    c.append(TrackCase('slide-plus-L2-2048', 2048, 10, 206, f_offset=3e6, carrier_hz=L2_HZ))
    c.append(TrackCase('many', 2048, 3, 207, sats=_sats(2048, range(8)),
                       chans=[(s, df) for s in range(8) for df in MANY_DF]))
    c.append(TrackCase('far', 2048, 10, 208))
    return {t.name: t for t in c}


TRACK_CASES = _build_track_cases()


def many_cut(case):
    """The sample count at which about half the channels of `many` fit two bits and not three: the
    median over the channels of the end of the third bit's last window."""
    ref, st, nk = case.ref()
    ends = sorted(int(nk[h, 2].max()) + case.cs + 1 for h in range(len(st)))
    return (ends[len(ends) // 2 - 1] + ends[len(ends) // 2]) // 2


def closest_to_integer(rec, st, nk, cs, **kw):
    """The closest approach of the restatement's s_k to an integer over every tracked bit."""
    worst = 1.0
    for h in range(len(st)):
        for b in range(st[h]['bit_no']):                # (every case starts from fresh channels)
            _, s, n = W.windows(rec[h, b]['tau'], rec[h, b]['f_hz'], cs, **kw)
            assert np.array_equal(n, nk[h, b])
            worst = min(worst, float(np.minimum(s - n, 1.0 - (s - n)).min()))
    return worst
