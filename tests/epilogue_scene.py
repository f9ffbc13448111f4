"""Scenes and state tables of the epilogue tests: rows the closed loop does not visit, drawn so that
the reference itself (epilogue_ref, from dump_ref's float64 dumps rounded to float32) shows every
case listed in coverage_gaps() -- checked on the CPU by test_epilogue_ref.py and on the kernels'
own dumps by test_gpu_trk_epilogue.py.

Geometry of dump_scene: [rows, 13] state rows and forced delays, channels 5 and 6 closed, row i
reads block i % 16.  The 16 blocks are dump_scene.signal_blocks (complex64) worked over on the
host: blocks 8 .. 15 are blocks 0 .. 7 rolled so that one satellite's code starts at sample 0 (a
forced delay 0 behind a carry: N_CYC + 1 dumps that carry signal), and code periods of every block
are multiplied by -1 after a pattern per block (none, one toggle, every third period, every
period), which puts bit edges on chosen dumps.  Every job is forced to the true delay of its
satellite; its carrier phase is calibrated with one float64 wipe-off (dump_ref at PHASE 0), so that a
row can be drawn aligned (the signal in the real part), in quadrature (the real part is noise and
the arctangent jumps between its ends: many unwrap steps even in eight dumps) or anywhere."""
import numpy as np

import dump_ref as dr
import dump_scene as ds
import epilogue_ref as er

ROWS = 48
ROLLED = (0, 1, 2, 3, 4, 7, 8, 0)          # the channel whose satellite block 8 + k puts at delay 0
OFFSETS = (30.0, 60.0, 120.0, 250.0, 400.0)
DF_LENS = (1, 7, 8, 9, 15, 16, 17, -1, 0)  # (-1, 0: df_no - 1, df_no)
F32 = np.float32


def _sat_of(c, sc):
    return sc.sats[c % len(sc.sats)]


def _true_delay(sat, b, cs, n_cyc):
    return int(round(sat.delay - sat.doppler / 1575.42e6 * b * cs * n_cyc)) % cs


def toggles(b, n_cyc):
    """The code periods at whose start block b changes sign."""
    kind = b % 4
    if kind == 0:
        return ()
    if kind == 1:
        return (1 + (5 * b) % (n_cyc - 1),)
    if kind == 2:
        return tuple(range(1 + b % 3, n_cyc, 3))
    return tuple(range(1, n_cyc))


def blocks(cs, n_cyc):
    """(16 complex64 blocks, shift [16]): block b is signal block b % 8 rolled left by shift[b]
    samples, with the sign pattern of toggles(b)."""
    def make():
        c64, _, sc = ds.signal_blocks(cs, n_cyc)
        out, shift = [], np.zeros(ds.NB, np.int64)
        for b in range(ds.NB):
            x = c64[b % 8].copy()
            if b >= 8:
                shift[b] = _true_delay(_sat_of(ROLLED[b - 8], sc), b % 8, cs, n_cyc)
                x = np.roll(x, -shift[b])
            sign = 1.0
            for k in range(n_cyc):
                if k in toggles(b, n_cyc):
                    sign = -sign
                if sign < 0:
                    x[k * cs:(k + 1) * cs] *= F32(-1)
            out.append(np.ascontiguousarray(x))
        return out, shift
    return ds.memo(('epilogue blocks', cs, n_cyc), make)


def _threshold_std(step):
    """A float32 s with float32(3) * s == step exactly, or None."""
    s = F32(step) / F32(3)
    for _ in range(4):
        for cand in (s, np.nextafter(s, F32(0)), np.nextafter(s, F32(np.inf))):
            if F32(3) * cand == F32(step):
                return cand
        s = np.nextafter(s, F32(0))
    return None


def table(cs, n_cyc):
    """(state table [ROWS, 13], forced delays, float32-rounded float64 dumps per live job
    {(i, c): complex64 [n_dumps]}), drawn once per config."""
    def make():
        blks, shift = blocks(cs, n_cyc)
        _, _, sc = ds.signal_blocks(cs, n_cyc)
        cfg = er.config(cs, n_cyc)
        tab, forced = ds.empty_table(ROWS)
        rng = np.random.default_rng([cs, n_cyc, 77])
        dumps, zero_jobs = {}, 0
        for i in range(ROWS):
            b = i % ds.NB
            for c in ds.LIVE:
                j = i * len(ds.LIVE) + ds.LIVE.index(c)
                st = tab[i, c]
                sat = _sat_of(c, sc)
                d = (_true_delay(sat, b % 8, cs, n_cyc) - int(shift[b])) % cs
                forced[i, c] = d
                st['prn'], st['delay'], st['nps'] = sat.prn, d, cs - d
                # ---- carrier: at the satellite's Doppler, or off it by tens to hundreds of Hz
                off = 0.0
                if d == 0:
                    zero_jobs += 1
                    m = zero_jobs % 4                      # (every fourth one aligned: an edge on the extra dump)
                    if m:                                  # an unwrap step of either sign on the extra dump
                        off = (400.0, 330.0, 250.0)[m - 1] * (1 if (zero_jobs // 4 + m) % 2 else -1)
                elif j % 5 >= 3:
                    off = OFFSETS[(j // 5) % len(OFFSETS)] * (1 if j % 5 == 3 else -1)
                freq = F32(np.clip(sat.doppler + off, cfg.min_freq, cfg.max_freq))
                st['freq'] = freq
                st['omega0'] = F32(2 * np.pi * float(freq)) if (i + c) % 2 else F32(0)
                st['phase_locked'] = 0 if j % 4 == 2 else 1
                # ---- one float64 wipe-off at PHASE 0 without a carry: the dumps at any PHASE follow
                st['phase'] = F32(0)
                st['prev_sum_re'] = st['prev_sum_im'] = F32(0)
                r0 = dr.dump_ref(blks[b], st, d, cs, n_cyc)
                nd, n1 = int(r0['n_dumps']), int(r0['first_len'])
                d0 = r0['dumps'][:nd]
                amp = float(np.mean(np.abs(d0[1:])))
                if off == 0.0 and j % 7 != 6:              # aligned: the signal in the real part
                    ang = np.angle(d0[1])
                    if j % 7 == 5:                         # in quadrature: the real part is noise, the
                        ang += np.pi / 2                   # arctangent jumps between its ends
                    phase = F32((ang + rng.normal() * 0.04 + (np.pi if j % 2 else 0.0)) % (2 * np.pi))
                else:
                    phase = (F32(0), ds.PHASE_TOP, F32(rng.uniform(0, 6.28)), F32(rng.uniform(0, 6.28)))[j % 4]
                st['phase'] = min(phase, ds.PHASE_TOP)
                rot = np.exp(-1j * float(st['phase']))
                body = d0[1:] * rot
                prev = complex(body[0]) * (cs - d) * (1 if j % 3 else -1)   # a carry like the dumps behind it
                st['prev_sum_re'], st['prev_sum_im'] = F32(prev.real), F32(prev.imag)
                prev = complex(float(st['prev_sum_re']), float(st['prev_sum_im']))
                g = np.concatenate([[(prev + d0[0] * n1 * rot) / n1], body]).astype(np.complex64)
                dumps[i, c] = g
                re = g.real
                # ---- the edge scan's words
                kind = j % 12
                sgn0 = 1.0 if re[0] > 0 else -1.0
                st['prev_signal'] = F32(amp * rng.uniform(0.5, 1.5) * (1 if rng.integers(0, 2) else -1))
                st['std_dev'] = F32(amp * rng.uniform(0.02, 0.2))
                st['edge_state'] = int(np.sign(st['prev_signal']))
                if kind == 0:                              # EDGES[0] not set yet
                    st['edge_state'] = 0
                elif kind == 1:                            # parked
                    st['edge_state'] = 2
                elif kind == 2:                            # prevSign against PREV_SIGNAL's sign
                    st['edge_state'] = -int(st['edge_state'])
                elif kind == 3:                            # an edge on dump 0
                    st['prev_signal'] = F32(-sgn0 * amp)
                    st['edge_state'] = int(-sgn0)
                    st['std_dev'] = F32(amp * 0.05)
                elif kind == 4:                            # PREV_SIGNAL exactly 0: dump 0 is no edge
                    st['prev_signal'] = F32(0)
                    st['edge_state'] = int(-sgn0)
                    st['std_dev'] = F32(0)
                elif kind == 5:                            # no threshold at all
                    st['std_dev'] = F32(0)
                elif kind == 6:                            # a threshold no step reaches
                    st['std_dev'] = F32(1.0)
                elif kind in (7, 8):                       # half the steps below 3 STD_DEV, half above
                    st['std_dev'] = F32(np.median(np.abs(np.diff(re))) / 3)
                elif kind == 9:                            # the step onto dump 0 exactly 3 STD_DEV: a
                    st['prev_signal'] = F32(-sgn0 * 16.0)  # PREV_SIGNAL so large that the step's last
                    st['edge_state'] = int(-sgn0)          # bit is far above a kernel's rounding of dump 0
                    s = _threshold_std(abs(F32(re[0] - st['prev_signal'])))
                    # (not every step is 3 x a float32; coverage_gaps asserts that some rows are)
                    st['std_dev'] = s if s is not None else F32(5.5)
                # ---- the drift list
                n = DF_LENS[(j // 4) % len(DF_LENS)]
                n = n + cfg.df_no if n <= 0 else n
                st['df_len'] = n if st['phase_locked'] else 1
                lst = rng.normal(size=n) * 0.05
                if j % 8 == 1:                             # a drift that the clamp cuts, either sign
                    lst += 1.5 * cfg.max_df * (1 if (j // 8) % 2 else -1)
                st['df'][:n] = lst.astype(F32)
                tab[i, c] = st
        tab['prn'][:, list(ds.CLOSED)] = 0
        return tab, forced, dumps
    return ds.memo(('epilogue table', cs, n_cyc), make)


def coverage_gaps(jobs, cs, n_cyc, ref=None):
    """What the reference shows on the jobs given -- [(state row, complex64 dumps, delay_used)] --
    against the list every table must reach; returns the items that are missing (empty: all
    there)."""
    ref = ref or er.Epilogue()
    cfg = er.config(cs, n_cyc)
    seen = set()
    for st, g, d in jobs:
        t = ref.tolerant64(st, g, cfg)
        x = ref.exact(st, g, d, cfg, F32(t['df']), F32(t['phase_shift']))
        locked0 = bool(st['phase_locked'])
        seen.add(('locked', locked0, bool(t['locked'])))
        for i in np.flatnonzero(t['steps']):
            seen.add(('step', int(t['steps'][i]), int(i)))
        if np.count_nonzero(t['steps']) >= 4:
            seen.add('4 steps')
        if abs(t['steps'].sum()) >= 2:
            seen.add(('net', int(np.sign(t['steps'].sum()))))
        seen.add(('freq', int(x['s_freq'] >= cfg.max_freq) - int(x['s_freq'] <= cfg.min_freq),
                  bool(x['s_omega0'] != 0), bool(st['omega0'] != 0)))
        seen.add(('phase', 0 if st['phase'] == 0 else 'top' if st['phase'] == ds.PHASE_TOP else 'any'))
        if not locked0:
            continue
        mask = x['o_edge_mask']
        n_edges = bin(mask).count('1')
        for i in range(len(g)):
            if mask >> i & 1:
                seen.add(('edge', i))
        seen.add(('edges', min(n_edges, 5) if n_edges not in (3, 4) else 3))
        seen.add(('edge_state0', int(st['edge_state']), x['o_edge_sign0']))
        seen.add(('prev_signal0', int(np.sign(st['prev_signal']))))
        re = g.real
        if st['std_dev'] == 0:
            seen.add('std_dev0 = 0')
        elif n_edges == 0 and np.any(np.diff(np.sign(re)) != 0) and F32(3) * st['std_dev'] > 2 * np.abs(re).max():
            seen.add('std_dev0 suppresses every edge')
        flips = np.flatnonzero(np.diff(np.sign(re)) != 0)
        steps = np.abs(np.diff(re))[flips]
        thr = F32(3) * st['std_dev']
        if np.any((steps[:-1] > thr) != (steps[1:] > thr)) and np.any(np.diff(flips) == 1):
            seen.add('a small step next to a large one')
        before = np.concatenate([[F32(st['prev_signal'])], re[:-1]])
        at_thr = (np.abs(re - before) == thr) & (np.sign(re) != np.sign(before))
        if thr > 0 and any(not mask >> int(i) & 1 for i in np.flatnonzero(at_thr)):
            seen.add('a step of exactly 3 std_dev0 is no edge')
        seen.add(('df_len', int(st['df_len'])))
        seen.add(('df clamp', t['clamped']))
        if len(g) == n_cyc + 1:
            seen.add(('extra dump', bool(mask >> n_cyc & 1)))
    want = [('locked', True, True), ('locked', False, False), ('locked', False, True),
            '4 steps', ('net', 1), ('net', -1), 'std_dev0 = 0', 'std_dev0 suppresses every edge',
            'a small step next to a large one', 'a step of exactly 3 std_dev0 is no edge', ('df clamp', 1), ('df clamp', -1), ('df clamp', 0),
            ('extra dump', True), ('edge_state0', 0, 1), ('edge_state0', 0, -1), ('edge_state0', 1, 0),
            ('edge_state0', -1, 0), ('edge_state0', 2, 0)]
    want += [('step', s, i) for s in (1, -1) for i in range(1, n_cyc + 1)]
    want += [('edge', i) for i in range(n_cyc + 1)]
    want += [('edges', k) for k in (0, 1, 2, 5)]
    want += [('prev_signal0', s) for s in (-1, 0, 1)]
    want += [('df_len', n) for n in {1, 7, 8, 9, 15, 16, 17, cfg.df_no - 1, cfg.df_no}]
    want += [('freq', e, e != 0, o) for e in (-1, 0, 1) for o in (False, True)]
    want += [('phase', p) for p in (0, 'top', 'any')]
    return [w for w in want if w not in seen]


def cpu_jobs(cs, n_cyc):
    """The live jobs of the table with dump_ref's dumps: [(state row, dumps, delay_used)]."""
    tab, forced, dumps = table(cs, n_cyc)
    return [(tab[i, c], dumps[i, c], int(forced[i, c])) for i in range(ROWS) for c in ds.LIVE]
