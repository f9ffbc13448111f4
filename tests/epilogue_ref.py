"""The tracking epilogue of one job restated on the CPU (csrc/gpsmi_trk_epilogue.h: edge scan,
amplitude statistics, phase unwrap, loop filter, carrier update, state row), shared by
test_epilogue_ref.py (CPU) and test_gpu_trk_epilogue.py (GPU).  Written from include/gpsmi.h and
the oracle (decode_data, phase_locked_loop and process of oracle/gps_oracle.py).

A job is its input state row, its prompt dumps (complex64, n_dumps of them) and its delay_used.
Two layers, kept apart:

  exact      fields that are IEEE float32 add / multiply / compare / fmod or integers: the edge
             scan, the carrier given the record's own df and phase_shift, the drift list given the
             record's own df, the copied words.  numpy float32, compared bitwise.
  toleranced std_dev, amplitude, phase_shift and df pass through hypot, atan, sqrt or a division:
             float64 from the same dumps (tolerant64), and the float32 oracle's arithmetic
             unchanged (tolerant_oracle: SatStream.phase_locked_loop, np.std / np.mean of np.abs on
             complex64), whose deviation from float64 gives the bounds.

Epilogue is a class so that test_epilogue_ref.py can apply one fault at a time to a copy (a
subclass that overrides one small method) and show that the tables notice."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
TWO_PI = F32(2 * np.pi)                  # float32(2 pi), numpy's weak-scalar cast
TOLERANCED = ('std_dev', 'amplitude', 'phase_shift', 'df')

_T_LAST = {}


def t_last(cs, n_cyc):
    """SEC_TIME[NGPS - 1] as the float32 the oracle holds."""
    if (cs, n_cyc) not in _T_LAST:
        import gps_oracle as orc
        _T_LAST[cs, n_cyc] = F32(orc.sec_time(orc.Params(code_samples=cs, n_cyc=n_cyc))[-1])
    return _T_LAST[cs, n_cyc]


def config(cs, n_cyc):
    """What the epilogue reads of the engine's Config (FREQ's clamp: its min_freq / max_freq)."""
    from gpsmi.engine import Config
    c = Config(code_samples=cs, n_cyc=n_cyc)
    return SimpleNamespace(cs=cs, n_cyc=n_cyc, df_no=1024 // n_cyc, min_freq=c.min_freq, max_freq=c.max_freq,
                           max_df=20.0 / (1024 // n_cyc), t_last=t_last(cs, n_cyc))


def parked_prev_sign(edge_state0):
    """prevSign at the start of a block.  edge_state 2 is 'prevSign is 0' (an edge onto a dump whose
    real part is exactly 0) and stays parked: no further edge until erasePrevData.  include/gpsmi.h
    documents this as a known deviation (the reference re-derives prevSign in every call); a change
    of that rule touches this function alone."""
    return 0 if edge_state0 == 2 else int(edge_state0)


class Epilogue:
    """The reference.  Every method is a pure function of its arguments."""

    # ---- exact layer

    def before(self, re, i, prev_signal0):
        """The real part the scan compares dump i with: the dump before, PREV_SIGNAL for dump 0."""
        return F32(prev_signal0) if i == 0 else re[i - 1]

    def carries_sign(self, p, prev):
        """prevSign * PREV_SIGNAL > 0: the dump before carried prevSign's sign."""
        return F32(p) * prev > 0

    def step_large(self, step, thr):
        return step > thr

    def mask_word(self, mask):
        return mask

    def edge_scan(self, re, prev_signal0, std_dev0, edge_state0):
        """decode_data's loop over the dumps of a locked job (re: float32 real parts).  Returns
        (edge mask, edge_sign0, next edge_state)."""
        thr = F32(3) * F32(std_dev0)
        p = parked_prev_sign(edge_state0)
        unset = edge_state0 == 0                          # EDGES[0] == 0
        sign0, mask = 0, 0
        for i, m in enumerate(re):
            sgn = int(np.sign(m))
            prev = self.before(re, i, prev_signal0)
            if unset:
                sign0 = p = sgn
                unset = sgn == 0
            elif (sgn != p and self.carries_sign(p, prev)
                  and self.step_large(abs(F32(m - prev)), thr)):
                mask |= 1 << i
                p = sgn
        state = 0 if unset else (2 if p == 0 else p)
        return self.mask_word(mask), sign0, state

    def carrier(self, st, df, phase_shift, cfg):
        """(freq, omega0, phase) of the next block from the record's own df and phase_shift."""
        freq0, om0 = F32(st['freq']), F32(st['omega0'])
        om = om0 if om0 != 0 else F32(TWO_PI * freq0)
        ph = F32(F32(st['phase']) + F32(om * cfg.t_last))
        mod = F32(np.fmod(ph, TWO_PI))
        if mod < 0:
            mod = F32(mod + TWO_PI)
        phase = F32(mod + F32(phase_shift))
        freq, omega0 = F32(freq0 + F32(df)), F32(0)
        if freq > F32(cfg.max_freq):
            freq, omega0 = F32(cfg.max_freq), F32(2 * np.pi * cfg.max_freq)
        elif freq < F32(cfg.min_freq):
            freq, omega0 = F32(cfg.min_freq), F32(2 * np.pi * cfg.min_freq)
        return freq, omega0, phase

    def list_full(self, n, df_no):
        return n >= df_no

    def shifted(self, lst):
        return lst[1:]

    def drift(self, st, df, cfg):
        """The next drift list (float32) from the record's own df and the lock flag of the input."""
        if not st['phase_locked']:
            return [F32(df)]
        lst = [F32(v) for v in st['df'][:int(st['df_len'])]]
        if self.list_full(len(lst), cfg.df_no):
            lst = self.shifted(lst)
        return lst + [F32(df)]

    def exact(self, st, dumps, delay_used, cfg, df, phase_shift):
        """Every exact field of the record ('o_*') and of the next state row ('s_*') but the two
        that are compared with the record's own (std_dev, phase_locked), as a dict."""
        re = np.asarray(dumps).real.astype(F32)
        r = {'s_prn': int(st['prn']), 's_delay': int(delay_used), 's_reserved': 0,
             'o_n_dumps': len(re), 'o_edge_mask': 0, 'o_edge_sign0': 0, 'o_ms_count': 0,
             's_edge_state': int(st['edge_state']), 's_prev_signal': F32(st['prev_signal'])}
        if st['phase_locked']:
            r['o_edge_mask'], r['o_edge_sign0'], r['s_edge_state'] = self.edge_scan(
                re, st['prev_signal'], st['std_dev'], int(st['edge_state']))
            r['o_ms_count'] = len(re)
            r['s_prev_signal'] = re[-1]
        freq, om, phase = self.carrier(st, df, phase_shift, cfg)
        r['o_freq'] = r['s_freq'] = freq
        r['o_phase'] = r['s_phase'] = phase
        r['s_omega0'] = om
        r['s_df'] = self.drift(st, df, cfg)
        r['s_df_len'] = len(r['s_df'])
        return r

    # ---- toleranced layer, float64

    def total(self, a):
        return np.sum(a)

    def unwrap_step(self, delta):
        return -np.sign(delta) if abs(delta) > 2.0 else 0.0

    def unwrap_range(self, n):
        return range(1, n)

    def neighbour(self, ph, i):
        return ph[i - 1]

    def clamp(self, df, max_df):
        return np.sign(df) * max_df

    def tolerant64(self, st, dumps, cfg):
        """std_dev, amplitude, phase_shift, df and the decisions (unwrap steps, df clamp, lock) in
        float64 from the float32 dumps, with the margin of every decision to its threshold."""
        d = np.asarray(dumps).astype(np.complex128)
        n = len(d)
        mag = np.hypot(d.real, d.imag)
        mean = self.total(mag) / n
        std = np.sqrt(self.total((mag - mean) ** 2) / n)
        ph = np.arctan(d.imag / d.real)
        steps, dp, real, m_step = np.zeros(n), 0.0, ph.copy(), np.inf
        for i in self.unwrap_range(n):
            delta = ph[i] - self.neighbour(ph, i)
            m_step = min(m_step, abs(abs(delta) - 2.0))
            steps[i] = self.unwrap_step(delta)
            dp += steps[i]
            real[i] += dp * np.pi
        offset = np.sum(real[-4:]) / 4
        dev = self.total(real) / n
        clamped, m_df = 0, np.inf
        if st['phase_locked']:
            k = int(st['df_len'])
            df = dev + self.total(np.asarray(st['df'][:k], np.float64)) / k
            m_df = abs(abs(df) - cfg.max_df)
            if abs(df) > cfg.max_df:
                df, clamped = self.clamp(df, cfg.max_df), int(np.sign(df))
        else:
            df = 10.0 * dev
        locked = bool(st['phase_locked']) or abs(dev) < 0.1
        m_lock = np.inf if st['phase_locked'] else abs(abs(dev) - 0.1)
        return {'std_dev': std, 'amplitude': mean / std, 'phase_shift': offset, 'df': df, 'dev': dev,
                'steps': steps, 'clamped': clamped, 'locked': int(locked),
                'm_step': m_step, 'm_df': m_df, 'm_lock': m_lock}


def tolerant_oracle(st, dumps, cfg):
    """The same fields with the float32 oracle's arithmetic, unchanged: SatStream.phase_locked_loop
    on a stand-in that carries the attributes it reads, np.std / np.mean of np.abs on complex64 (as
    SatStream.process).  test_oracle.py pins that arithmetic to the reference."""
    import gps_oracle as orc
    d = np.asarray(dumps, np.complex64)
    k = int(st['df_len'])
    ss = SimpleNamespace(no_sec=cfg.df_no, phase_locked=bool(st['phase_locked']),
                         df=[F32(v) for v in st['df'][:k]],
                         DF_GAIN1=orc.SatStream.DF_GAIN1, DF_GAIN2=orc.SatStream.DF_GAIN2)
    with np.errstate(divide='ignore'):
        df, offset, locked, real = orc.SatStream.phase_locked_loop(ss, d)
        ph = np.arctan(d.imag / d.real)
    std = np.std(np.abs(d))
    assert std.dtype == F32 and np.asarray(df).dtype == F32 and np.asarray(offset).dtype == F32
    steps = np.diff(np.rint((real.astype(np.float64) - ph) / np.pi), prepend=0.0)
    clamped = int(np.sign(df)) if ss.phase_locked and abs(df) == F32(cfg.max_df) else 0
    return {'std_dev': std, 'amplitude': np.mean(np.abs(d)) / std, 'phase_shift': offset, 'df': df,
            'steps': steps, 'clamped': clamped, 'locked': int(bool(locked)), 'df_list': list(ss.df)}


def deviation(got, ref):
    """How far a float32 realisation's toleranced fields are from the float64 ones: relative for
    std_dev and amplitude (positive scales), absolute for phase_shift and df (radians, Hz)."""
    out = {}
    for k in TOLERANCED:
        e = abs(float(got[k]) - float(ref[k]))
        out[k] = e / abs(float(ref[k])) if k in ('std_dev', 'amplitude') else e
    return out


def same_decisions(got, ref):
    return (np.array_equal(got['steps'], ref['steps']) and got['clamped'] == ref['clamped']
            and got['locked'] == ref['locked'])


def near_threshold(ref, bounds):
    """A threshold quantity of the float64 job lies within the bound of the field it decides:
    |delta ph| - 2 within phase_shift's, |mean phase| - 0.1 and |df| - max_df within df's."""
    return bool(ref['m_step'] <= bounds['phase_shift'] or ref['m_lock'] <= bounds['df']
                or ref['m_df'] <= bounds['df'])


def oracle_bounds(refs, orcs):
    """Per toleranced field 4 x the oracle's worst deviation from float64 over the jobs given
    (lists of tolerant64 / tolerant_oracle dicts), measured on the jobs where the oracle took
    float64's decisions.  Every other job must be near a threshold and counts as left out.
    Returns (bounds, worst figures, indices left out, failures): a figure that is not positive (NaN
    included) and an oracle that decides otherwise far from a threshold are failures, returned and
    not raised, so that a caller can print what it has before it fails."""
    same = [same_decisions(o, r) for o, r in zip(orcs, refs)]
    devs = [deviation(o, r) for o, r, s in zip(orcs, refs, same) if s]
    worst = {k: float(np.max([d[k] for d in devs])) if devs else float('nan') for k in TOLERANCED}
    failures = [('oracle figure not positive', k, v) for k, v in worst.items() if not v > 0]
    bounds = {k: 4 * v for k, v in worst.items()}
    out = [i for i, s in enumerate(same) if not s]
    failures += [('the oracle decides otherwise far from a threshold', i)
                 for i in out if not near_threshold(refs[i], bounds)]
    return bounds, worst, out, failures


def job_dumps(rec):
    """complex64 prompt dumps of one gpsmi_trk_out record, bytewise (engine.dumps_of)."""
    from gpsmi.engine import dumps_of
    return dumps_of(rec)


def compare_job(ref, st, rec, nxt, delay_used, cfg, bounds):
    """One live job of a kernel form against the reference, from the kernel's own dumps.
    Returns (failures, deviations or None, left out, tolerant64).  Failures: exact mismatches
    (field, got, want), a toleranced field that is not finite, and every toleranced field that is not
    within its bound -- `not (dev <= bound)`, so that NaN fails.  A job is left out (deviations None)
    only with finite fields, next to a threshold."""
    dumps = job_dumps(rec)
    want = ref.exact(st, dumps, delay_used, cfg, rec['df'], rec['phase_shift'])
    bad = []

    def same(name, got, exp):
        a, b = np.asarray(got), np.asarray(exp, dtype=np.asarray(got).dtype)
        if a.tobytes() != b.tobytes():
            bad.append((name, got, exp))

    if int(rec['n_dumps']) != want['o_n_dumps']:
        bad.append(('n_dumps', int(rec['n_dumps']), want['o_n_dumps']))
    same('edge_mask', rec['edge_mask'], want['o_edge_mask'] & 0xFFFFFFFF)
    same('edge_mask_hi', rec['edge_mask_hi'], want['o_edge_mask'] >> 32)
    for k in ('edge_sign0', 'ms_count', 'freq', 'phase'):
        same(k, rec[k], want['o_' + k])
    same('reserved1', rec['reserved1'], 0)
    for k in ('prn', 'delay', 'reserved', 'edge_state', 'prev_signal', 'freq', 'phase', 'omega0', 'df_len'):
        same('next ' + k, nxt[k], want['s_' + k])
    same('next df', nxt['df'][:want['s_df_len']], np.asarray(want['s_df'], F32))
    same('next std_dev == std_dev', nxt['std_dev'], rec['std_dev'])
    same('next phase_locked == phase_locked', nxt['phase_locked'], rec['phase_locked'])
    same('next nps == nps', nxt['nps'], rec['nps'])
    r64 = ref.tolerant64(st, dumps, cfg)
    dev = deviation(rec, r64)
    finite = True
    for k in TOLERANCED:
        if not np.isfinite(rec[k]):
            bad.append((k, rec[k], 'not finite'))
            finite = False
    within = int(rec['phase_locked']) == r64['locked'] and all(dev[k] <= bounds[k] for k in TOLERANCED)
    if finite and not within and near_threshold(r64, bounds):
        return bad, None, True, r64                       # decided otherwise next to a threshold
    if int(rec['phase_locked']) != r64['locked']:
        bad.append(('phase_locked', int(rec['phase_locked']), r64['locked']))
    for k in TOLERANCED:
        if not dev[k] <= bounds[k]:
            bad.append((k, 'deviation', dev[k], 'bound', bounds[k]))
    return bad, dev, False, r64
