"""The calls of cancellation, signatures and profiles at which the window
rule (csrc/gpsmi_windows.h) and the kernels behind it do what the short kernel scenes never ask of
them, and the scenes they run on: shared by test_windows_cases.py (CPU: every call is what its name
says) and test_gpu_windows_long.py (GPU: the kernels against the float64 restatements on them).

  slip   n = 21 cs + 123.  The starts j_k = rint(tau + k Tc) of a record are cs apart only while the
         fraction of tau + k Tc stays on one side of a half: `natural` lets L1's own code Doppler carry
         it across; `fast` / `slow` take a carrier of 400 kHz (scale 1.00774 / 0.99025: a period of 2032
         or 2068 samples at 2048, so every few periods one is a sample longer); `offset_*` reach the same
         through f_offset_hz, and `offset_slow` holds a record at 0.44 fs beside it.
  many   300 code periods at 2048, 19 at 16368, and their heads: the same rows and records cut to
         257 and 9 (17 and 9) periods.  A record's windows are ALL the periods that lie inside the rows
         -- tau names any one code start, it does not cut the periods before it -- so the records of
         one call differ by a window at the most: 300 / 299, 257 / 256, 9 / 8.  That is what the
         kernels' paths need: groups of prompts behind the first, a partial last group, a record
         whose last workgroup finds nothing to do (256 and 8 beside 257 and 9), a second window per
         thread of the covariance (257: exactly one thread has one), some 300 runs of profiles.
  late   1004 code periods at 2048: the last windows start two million samples in, and both
         satellites are cancelled over the whole of it.

A record's satellite sits on its windows: with s = 1 + (f_hz - f_offset) / carrier_hz the code of a
synth.Sat restarts every cs / (1 - delay_rate) samples from delay / (1 - delay_rate) on, so delay_rate =
1 - s and delay = tau s.  (1 / s - 1 is the same to first order only: at s = 1.00774 it is 6e-5 of a
period off, 2.6 samples after 21 periods.)  Where s is 1 % from 1 the satellite's code slides 16 samples
along the unstretched replica within one window, so its prompts are no larger than the noise's: those
calls are about where the windows lie, not about the satellite.  Amplitude 0.11 and noise 0.35 as in the
kernel scenes of cancel_ref / sig_ref / profile_ref.  Everything rendered or restated here is cached and
read-only."""
import functools
from typing import NamedTuple

import numpy as np

import cancel_ref as CR
import profile_ref as PR
import sig_ref as SR
from cancel_ref import L1_HZ

SMALL_CARRIER = 4.0e5
KSIG_GROUP = 8                    # kSigWinPerWg: the windows of one workgroup of sig_prompt_kernel
KSIG_STRIDE = 256                 # the threads of sig_cov_kernel: window 256 is a thread's second
SINES = (-0.7, 0.2, 0.85)


class Call(NamedTuple):
    """One call's arguments: rows of n samples, the records (prn, f_hz, tau) and the two options every
    stage takes."""
    name: str
    cs: int
    n: int
    antennas: int                 # the rows the scene is rendered with
    carrier_hz: float
    f_offset: float
    records: tuple
    seed: int
    rendered_n: int = 0           # a head: the length of the rows it is cut from (0: n)
    scene_records: tuple = ()     # other records on the same rows: the records the rows were rendered for

    @property
    def opts(self):
        return dict(carrier_hz=self.carrier_hz, f_offset=self.f_offset)

    @property
    def id(self):
        return '%s-%d' % (self.name, self.cs)

    def scale(self, f_hz):
        return 1.0 + (f_hz - self.f_offset) / self.carrier_hz

    def prof_records(self, skip=0, prns=None):
        """The records as profiles take them, (prn, skip_ms, f_hz, tau); prns: only those."""
        return [(p, skip, f, tau) for p, f, tau in self.records if prns is None or p in prns]

    def on_the_same_rows(self, records):
        return self._replace(records=tuple(records), scene_records=self.scene_records or self.records)

    def head(self, n):
        """The same records on the first n samples of the same rows."""
        return self._replace(name='%s_head%d' % (self.name, n // self.cs), n=n, rendered_n=self.rendered_n or self.n)


# ---- the calls ----------------------------------------------------------------------------------
SLIP_NAMES = ('natural', 'fast', 'slow', 'offset_fast', 'offset_slow')
# the steps between consecutive signature starts, {prn: steps}, as a CPU run of the restatements gave
# them when the cases were set
SLIP_STEPS = {('natural', 2048): {5: {2048, 2049}, 4: {2048}}, ('natural', 16368): {5: {16368, 16369}},
              ('fast', 2048): {4: {2032, 2033}}, ('fast', 16368): {4: {16242, 16243}},
              ('slow', 2048): {5: {2068, 2069}}, ('slow', 16368): {5: {16529, 16530}},
              ('offset_fast', 2048): {4: {2032, 2033}}, ('offset_fast', 16368): {4: {16244, 16245}},
              ('offset_slow', 2048): {4: {2066, 2067}, 9: {2065, 2066}},
              ('offset_slow', 16368): {4: {16514, 16515}, 9: {16438, 16439}}}


def slip(name, cs):
    k = cs / 2048.0
    table = {'natural': (L1_HZ, 0.0, ((4, 3096.0, 15.003), (5, -4319.0, 700.4968))),
             'fast': (SMALL_CARRIER, 0.0, ((4, 3096.0, 0.3),)),
             'slow': (SMALL_CARRIER, 0.0, ((5, -3900.0, cs - 0.3),)),
             'offset_fast': (L1_HZ, -1.2e7, ((4, 3096.0, 100.25),)),
             # the second record: f_hz = 0.44 fs, where the carrier turns by 0.88 pi a sample; +1.4e7 keeps
             # its scale inside (0.99, 1.01) at both rates (0.99169 and 0.99568), -1.2e7 would not at 16368
             'offset_slow': (L1_HZ, 1.4e7, ((4, 3096.0, 100.25), (9, 440.0 * cs, 1347.4 * k)))}
    carrier, off, rec = table[name]
    return Call(name, cs, 21 * cs + 123, 2, carrier, off, rec, 41 + SLIP_NAMES.index(name))


def many(cs):
    if cs == 2048:
        rec = ((4, 3096.0, 0.3), (5, -4319.0, 291 * cs + 0.3), (9, 402.0, 43 * cs + 700.2))
        return Call('many', cs, 300 * cs + 77, 8, L1_HZ, 0.0, rec, 53)
    rec = ((4, 3096.0, 0.3), (5, -4319.0, 2 * cs + 0.3), (9, 402.0, 9 * cs + 700.2 * cs / 2048.0))
    return Call('many', cs, 19 * cs + 50, 4, L1_HZ, 0.0, rec, 59)


# the lengths the many-window rows are called at, and the windows of each record there
MANY_N = {2048: (300 * 2048 + 77, 257 * 2048 + 77, 9 * 2048 + 5), 16368: (19 * 16368 + 50, 17 * 16368 + 50, 9 * 16368 + 50)}
MANY_WINDOWS = {2048: ([300, 299, 299], [257, 256, 256], [9, 8, 8]), 16368: ([19, 19, 18], [17, 17, 16], [9, 9, 8])}
STALE_N = 19 * 2048 + 50          # what runs on a 2048 handle straight after the 300-window call


def many_at(cs, n):
    c = many(cs)
    return c if n == c.n else c.head(n)


def late():
    cs = 2048
    rec = ((4, 3096.0, 1000 * cs + 0.3), (5, -4319.0, 1000 * cs + 700.4))
    return Call('late', cs, 1004 * cs + 50, 2, L1_HZ, 0.0, rec, 61)


def all_calls():
    return [slip(nm, cs) for cs in (2048, 16368) for nm in SLIP_NAMES] + \
        [many_at(cs, n) for cs in (2048, 16368) for n in MANY_N[cs]] + [many_at(2048, STALE_N), late()]


class Prof(NamedTuple):
    """The options of one profile call on a Call's row 0."""
    Lh: int
    coh: int
    skip: int = 0
    n_runs: int = 0

    @property
    def kw(self):
        return dict(half_taps=self.Lh, coh_ms=self.coh, n_runs=self.n_runs)


def prof_settings(call):
    """The profile calls of a Call.  slip: runs of 5 windows -- a sample's slip falls inside a run, and
    the fifth window is a second trip of one wave alone -- in the rate's default build, single windows
    in the other; many: about 300 runs of one window in both builds and 14 of 20 windows with skip_ms 0
    and 7 (2048), 6 runs of 3 (16368); late: the first run alone, and all 334."""
    base = call.name.split('_head')[0]
    if base in SLIP_NAMES:
        return [Prof(8, 5), Prof(32, 1)] if call.cs == 2048 else [Prof(32, 5), Prof(5, 1)]
    if base == 'many':                             # (a head of 9 periods holds no run of 20)
        long = [] if call.rendered_n else [Prof(8, 20), Prof(8, 20, 7)]
        return [Prof(8, 1), Prof(32, 1)] + long if call.cs == 2048 else [Prof(32, 3), Prof(5, 3)]
    return [Prof(8, 3, 0, 1), Prof(8, 3)]


# ---- the windows, by the restatements ------------------------------------------------------------
def sig_starts(call, n_ms=0):
    return [SR.sig_windows(call.n, call.cs, f, tau, n_ms, **call.opts) for _, f, tau in call.records]


def prof_starts(call, Lh, coh, skip=0, n_runs=0, prns=None):
    return [PR.prof_windows(call.n, call.cs, f, tau, Lh, skip, coh, n_runs, **call.opts)
            for _, _, f, tau in call.prof_records(skip, prns)]


def cancel_wins(call):
    """Per record [(lo, hi, j, r0)]: cancel_ref's windows and the replica point of sample lo, (lo - j) mod cs."""
    return [[(lo, hi, j, (lo - j) % call.cs) for lo, hi, j in CR.cancel_windows(call.n, call.cs, f, tau, **call.opts)]
            for _, f, tau in call.records]


def steps(starts):
    return set(np.diff(np.asarray(starts, np.int64)).tolist())


# ---- the scenes ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rendered(call):
    from gpsmi import synth, synth_array
    sats = [synth.Sat(prn=p, doppler=f - 2.0, delay=tau * call.scale(f), amp=0.11, phase0=0.4 * i,
                      delay_rate=1.0 - call.scale(f)) for i, (p, f, tau) in enumerate(call.records)]
    sc = synth.Scene(sats=sats, seed=call.seed, noise_sigma=0.35, code_samples=call.cs)
    arr = synth_array.ArrayScene(sc, synth_array.ula_steering(call.antennas, SINES[:len(sats)]))
    out = arr.block_raw(0, n=call.n)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _decoded(call):
    from gpsmi.synth import raw_to_c64
    out = raw_to_c64(_rendered(call))
    out.setflags(write=False)
    return out


def _whole(call):
    """The call whose rows a call reads: a head reads the rows it is cut from."""
    return call._replace(name=call.name.split('_head')[0], n=call.rendered_n or call.n, rendered_n=0,
                         records=call.scene_records or call.records, scene_records=())


def raw(call):
    """uint16 [antennas][n]: the call's scene as every antenna's recorder wrote it, read-only."""
    return _rendered(_whole(call))[:, :call.n]


def c64(call):
    return _decoded(_whole(call))[:, :call.n]


def rows(call, A, raw_u8):
    """The first A rows (A = 0: row 0 alone, [n]) in an input format, contiguous."""
    x = (raw if raw_u8 else c64)(call)
    return np.ascontiguousarray(x[0] if A == 0 else x[:A])


# ---- the restatements of the calls --------------------------------------------------------------
def _frozen(res):
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def sig_reference(call, A, n_ms=0):
    """(P, C, n_win) of sig_ref.sig_ref over the first A rows."""
    return _frozen(SR.sig_ref(c64(call)[:A], list(call.records), call.cs, n_ms, **call.opts))


@functools.lru_cache(maxsize=None)
def prof_reference(call, Lh, coh, n_runs=0, skip=0, prns=None, plain32=False):
    """(S, Q, n_runs) of profile_ref.prof_ref over row 0."""
    return _frozen(PR.prof_ref(c64(call)[0], call.prof_records(skip, prns), call.cs, Lh, coh, n_runs,
                               plain32=plain32, **call.opts))


@functools.lru_cache(maxsize=None)
def cancel_reference(call):
    """(y, records, coef, processed) of cancel_ref.cancel_ref over row 0."""
    return _frozen(CR.cancel_ref(c64(call)[0], list(call.records), call.cs, **call.opts))
