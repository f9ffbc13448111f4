"""Scenes and job tables of the prompt-dump tests: what test_dump_ref.py (CPU) holds against the
oracle and test_gpu_trk_dumps.py (GPU) runs through every form of the correlators, with the
float64 and oracle records of every job (computed once per table and process).

A table is [rows, 13] state rows and forced delays; row i reads block i % 16 of its scene, so a
launch of 16 consecutive rows reads the scene's 16 blocks in order.  Thirteen channels are two
channel groups of the span correlators (twelve columns and one) and three of the vector one;
channels 5 and 6 are closed."""
import numpy as np

import corr_ref as cr
import dump_ref as dr

# (CODE_SAMPLES, N_CYC): the span correlator's three block lengths, trk_span8 / the chunked vector
# kernel, the vector kernel in two chunks
CONFIGS = ((2048, 32), (2048, 16), (2048, 8), (16368, 8), (4096, 16))
NB, NCH = 16, 13
NB_SMALL = 8                          # rows of the carry and signal tables
CLOSED = (5, 6)
LIVE = tuple(c for c in range(NCH) if c not in CLOSED)
PRNS = (3, 8, 11, 14, 19, 0, 0, 22, 26, 30, 31, 2, 5)
FREQS = (-5000.0, 5000.0, 0.0, -1234.5, 2871.25)
PHASE_TOP = np.nextafter(np.float32(2 * np.pi), np.float32(0))     # the largest float32 below 2 pi

# Forced delays: every place a correlator treats specially.
# CS = 2048, the list of test_forced_delays_at_every_edge_agree_across_correlators: the residues mod 4
# (K-steps of four positions), the edges of a 64-position tile, of a 512-position quarter (the vector
# kernel's wave), of the code period.
# CS = 16368: pairs and steps of four positions, trk_span8's tiles of 48, its re-seed every four tiles
# (192), its ranges of 528 (the first, one in the middle, the last: 15840 = 30 * 528); the vector
# kernel's chunks of 128 and waves of 512 positions and its launches of 2048 (the last one, from
# 14336, is short).
# CS = 4096: the vector kernel's chunks, waves and its two launches of 2048 positions.
EDGES = {
    2048: (0, 1, 2, 3, 4, 5, 6, 7, 61, 62, 63, 64, 65, 66, 67, 127, 128, 129, 130, 131, 255, 256, 257,
           509, 510, 511, 512, 513, 514, 515, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 1535, 1536, 1537,
           2040, 2041, 2042, 2043, 2044, 2045, 2046, 2047),
    16368: (0, 1, 2, 3, 4, 5, 6, 7, 46, 47, 48, 49, 50, 127, 128, 129, 190, 191, 192, 193, 511, 512, 513,
            526, 527, 528, 529, 530, 1055, 1056, 1057, 2047, 2048, 2049, 8183, 8184, 8185, 14335, 14336,
            14337, 15838, 15839, 15840, 15841, 16361, 16363, 16366, 16367),
    4096: (0, 1, 2, 3, 4, 5, 6, 7, 126, 127, 128, 129, 255, 256, 257, 510, 511, 512, 513, 514, 1023, 1024,
           1025, 2045, 2046, 2047, 2048, 2049, 2050, 2559, 2560, 2561, 3071, 3072, 3073, 3583, 3584, 3585,
           4088, 4089, 4090, 4091, 4092, 4093, 4094, 4095, 1535, 1537),
}

# the three carriers of the boundary-sensitive scene: (prn, Hz), code start at sample 0
CARRIERS = ((3, -5000.0), (8, 5000.0), (11, 0.0))

_CACHE = {}


def memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def boundary_blocks(cs, n_cyc):
    """(complex64 blocks, raw uint16 blocks) of the boundary-sensitive scene: both bytes of every
    raw sample lie in 0..63 or 192..255, so every component of every sample has a magnitude of at
    least 0.49 and one sample more or less in a window shows in its dump.  Which of the two ranges a
    byte takes is the sign of three carriers (CARRIERS, amplitude 0.5 each) in Gaussian noise; where
    in the range it lies is drawn.  The complex64 block is the decode of the raw one, bit for bit."""
    def make():
        rng = np.random.default_rng([cs, n_cyc, 6363])
        n = cs * n_cyc
        t = (np.arange(n, dtype=np.float64) + 1.0) / (1000.0 * cs)
        sig = sum(0.5 * np.tile(dr.replica(prn, cs), n_cyc) * np.exp(1j * (0.9 * i + 2 * np.pi * f * t))
                  for i, (prn, f) in enumerate(CARRIERS))
        raws = []
        for _ in range(NB):
            s = sig + 0.6 * (rng.normal(size=n) + 1j * rng.normal(size=n))
            depth = rng.integers(0, 64, (2, n))
            i8 = np.where(s.real > 0, 255 - depth[0], depth[0]).astype(np.uint16)
            q8 = np.where(s.imag > 0, 255 - depth[1], depth[1]).astype(np.uint16)
            raws.append((q8 << 8) | i8)
        c64 = [cr.decode_u8(r) for r in raws]
        for x in c64:
            assert min(np.abs(x.real).min(), np.abs(x.imag).min()) >= 0.49
        return c64, raws
    return memo(('boundary', cs, n_cyc), make)


def signal_blocks(cs, n_cyc):
    """(complex64 blocks, raw uint16 blocks, the scene) of the satellites of test_gpu_trk_corr.py
    (delays scaled to the code length), blocks 0 .. 7."""
    def make():
        from gpsmi import synth
        from test_gpu_trk_corr import SATS
        sc = synth.Scene(sats=[synth.Sat(prn=p, doppler=f, delay=d * cs / 2048.0, amp=a, phase0=0.7 * i)
                               for i, (p, f, d, a) in enumerate(SATS)],
                         seed=5200 + n_cyc, code_samples=cs, n_cyc=n_cyc)
        raws = [sc.block_raw(b) for b in range(NB_SMALL)]
        return [cr.decode_u8(r) for r in raws], raws, sc
    return memo(('signal', cs, n_cyc), make)


def template_row():
    """A state row as gpsmi_trk_open leaves it (every field the kernels range-check)."""
    from gpsmi.engine import STATE_DTYPE
    row = np.zeros((), STATE_DTYPE)
    row['df_len'] = 1
    row['std_dev'] = 0.005
    return row


def empty_table(rows):
    from gpsmi.engine import STATE_DTYPE
    table = np.empty((rows, NCH), STATE_DTYPE)
    table[...] = template_row()
    table['prn'] = PRNS
    return table, np.zeros((rows, NCH), np.int32)


def _carrier(st, rng, i, c):
    """FREQ over -5000, +5000, 0 and two values between, every one in every column; omega0 (the
    Python-float FREQ of a loop's first blocks) on half the rows; PHASE 0, the top, anywhere."""
    f = FREQS[(i + c) % len(FREQS)]
    st['freq'] = np.float32(f)
    st['omega0'] = np.float32(2 * np.pi * f) if (i + c // len(FREQS)) % 2 else np.float32(0)
    st['phase'] = (np.float32(0), PHASE_TOP, np.float32(rng.uniform(0, 6.28)),
                   np.float32(rng.uniform(0, 6.28)))[(i * NCH + c) % 4]


def _same_carrier(a, b):
    return all(a[k] == b[k] for k in ('prn', 'freq', 'omega0', 'phase'))


def _carry(st, rng, nps, scale=3.0):
    st['nps'] = nps
    st['prev_sum_re'] = np.float32(rng.normal() * scale)
    st['prev_sum_im'] = np.float32(rng.normal() * scale)


def edge_table(cs, n_cyc):
    """One row per entry of EDGES[cs]; column c of row i is forced to edge (i + 7 c) mod E, so every
    edge meets every column.  A third of the jobs start without a carry (nps = 0: the first window
    is the d samples in front of the boundary); the others carry CS - d + (-3 .. 3) samples and a
    drawn prev_sum, as behind a block whose delay was within three samples of this one (first
    windows of CS - 3 .. CS + 3 samples)."""
    def make():
        edges = EDGES[cs]
        assert all(0 <= e < cs for e in edges) and len(set(edges)) == len(edges)
        table, forced = empty_table(len(edges))
        rng = np.random.default_rng([cs, n_cyc, 1])
        for i in range(len(edges)):
            for c in LIVE:
                st = table[i, c]
                d = edges[(i + 7 * c) % len(edges)]
                forced[i, c] = d
                if i < NB:
                    _carrier(st, rng, i, c)
                else:                                      # the rows that read a block share its wipe-off
                    for k in ('freq', 'omega0', 'phase'):
                        st[k] = table[i - NB, c][k]
                st['delay'] = int(rng.integers(0, cs))
                if (i + 2 * c) % 3:
                    _carry(st, rng, int(np.clip(cs - d + rng.integers(-3, 4), 1, cs)))
                table[i, c] = st
        for c in LIVE:
            assert set(forced[:, c]) == set(edges)
        return table, forced
    return memo(('edge', cs, n_cyc), make)


CARRY_KINDS = 6


def carry_table(cs, n_cyc):
    """8 x 13 jobs of the state kinds of random_state_runs (test_gpu_trk.py) and the ends of their
    ranges, kind = job number mod 6:
      0  nps = 0, d = 0: the rows are the windows; the drawn prev_sum belongs to no sample
      1  nps > 0, d = 0: N_CYC + 1 dumps, the first one the carry alone
      2  nps + d > CS: a first window of more than a code period
      3  nps = CS (with d = 0 on every other one: the first dump is prev_sum / CS)
      4  nps and d of 1 .. 3 samples: a first window of a few samples, where a wrong divisor shows most
      5  nps and d anywhere
    with a drawn prev_sum of a few units wherever nps > 0."""
    def make():
        table, forced = empty_table(NB_SMALL)
        rng = np.random.default_rng([cs, n_cyc, 2])
        for i in range(NB_SMALL):
            for c in LIVE:
                st = table[i, c]
                j = i * len(LIVE) + LIVE.index(c)
                kind = j % CARRY_KINDS
                _carrier(st, rng, i, c)
                st['delay'] = int(rng.integers(0, cs))
                if kind == 0:
                    nps, d = 0, 0
                elif kind == 1:
                    nps, d = int(rng.integers(1, cs)), 0
                elif kind == 2:
                    nps = int(rng.integers(cs // 2, cs + 1))
                    d = int(rng.integers(cs - nps + 1, cs))
                elif kind == 3:
                    nps, d = cs, (0 if (j // CARRY_KINDS) % 2 else int(rng.integers(1, cs)))
                elif kind == 4:
                    nps, d = int(rng.integers(1, 4)), int(rng.integers(0, 4))
                else:
                    nps, d = int(rng.integers(1, cs + 1)), int(rng.integers(0, cs))
                _carry(st, rng, nps)
                forced[i, c] = d
                table[i, c] = st
        return table, forced
    return memo(('carry', cs, n_cyc), make)


def signal_table(cs, n_cyc):
    """8 x 13 jobs on signal_blocks: column c tracks satellite c mod 9 at its Doppler, with the
    window boundary at the true code start of the block + (-2 .. 2) samples and the carry of a
    block before with the same delay."""
    def make():
        from test_gpu_trk_corr import SATS
        _, _, sc = signal_blocks(cs, n_cyc)
        table, forced = empty_table(NB_SMALL)
        rng = np.random.default_rng([cs, n_cyc, 3])
        offs = np.zeros((NB_SMALL, NCH), np.int32)
        for i in range(NB_SMALL):
            for c in LIVE:
                st = table[i, c]
                sat = sc.sats[c % len(SATS)]
                true = sat.delay - sat.doppler / 1575.42e6 * i * cs * n_cyc
                offs[i, c] = (i + c) % 5 - 2
                d = (int(round(true)) + offs[i, c]) % cs
                st['prn'] = sat.prn
                st['freq'] = np.float32(sat.doppler)
                st['omega0'] = np.float32(2 * np.pi * sat.doppler) if i % 2 else np.float32(0)
                st['phase'] = np.float32(rng.uniform(0, 6.28))
                st['delay'] = d
                _carry(st, rng, cs - d, 1.0)
                forced[i, c] = d
                table[i, c] = st
        table['prn'][:, list(CLOSED)] = 0
        return table, forced, offs
    return memo(('signal table', cs, n_cyc), make)


def references(blocks, table, forced, cs, n_cyc, key):
    """(float64 records, oracle records) [rows, 13] of a table on its scene (closed channels: zero
    records), computed once per key."""
    def make():
        ref = np.zeros(table.shape, dr.DUMP_DTYPE)
        orc = np.zeros(table.shape, dr.DUMP_DTYPE)
        for b in range(min(NB, table.shape[0])):
            for c in LIVE:
                first = table[b, c]                        # the wipe-offs, once per (block, carrier)
                wiped = dr.wipe(blocks[b], first, cs, n_cyc), dr.oracle_wipe(blocks[b], first, cs, n_cyc)
                for i in range(b, table.shape[0], NB):
                    if i > b and not _same_carrier(table[i, c], first):
                        wiped = dr.wipe(blocks[b], table[i, c], cs, n_cyc), dr.oracle_wipe(blocks[b], table[i, c], cs, n_cyc)
                    args = (blocks[b], table[i, c], int(forced[i, c]), cs, n_cyc)
                    ref[i, c] = dr.dump_ref(*args, wiped=wiped[0])
                    orc[i, c] = dr.oracle_record(*args, wiped=wiped[1])
        return ref, orc
    return memo(('references', key, cs, n_cyc), make)


def engine(cs, n_cyc, family, prns):
    """A TrkEngine whose prompt correlator is the family asked for ('vector', or the span / span8
    correlator the handle chooses by default), asserted through get_option."""
    from gpsmi import engine as E
    cfg = E.Config(code_samples=cs, n_cyc=n_cyc)
    if family != 'vector':
        eng = E.TrkEngine(cfg, max_ch=NCH, prns=prns)
        assert eng.get_option('correlator') == 1, (cs, n_cyc, family)
        return eng
    E.set_default('correlator', 0)
    try:
        eng = E.TrkEngine(cfg, max_ch=NCH, prns=prns)
    finally:
        E.clear_default('correlator')
    assert eng.get_option('correlator') == 0, (cs, n_cyc)
    return eng


def replay(eng, buf, nbytes, table, forced):
    """The table in launches of at most 16 rows (row i reads block i % 16 of the buffer)."""
    outs, nxts = [], []
    for r0 in range(0, table.shape[0], NB):
        nb = min(NB, table.shape[0] - r0)
        outs.append(eng.replay(buf.ptr, nb, table[r0:r0 + nb], forced[r0:r0 + nb]))
        nxts.append(eng.replay_states(nb))
    return np.concatenate(outs), np.concatenate(nxts)


def live(a):
    """The live columns of a [rows, 13] array, flat."""
    return np.ascontiguousarray(a[:, list(LIVE)]).ravel()


def bounds(orc, ref):
    """Per field 4 x the oracle's worst deviation from float64 over the jobs given (flat arrays),
    with the figures themselves.  The integer fields of the two must agree on every job."""
    for k in dr.INTS:
        assert np.array_equal(orc[k], ref[k]), k
    dev = dr.deviations(orc, ref)
    worst = {k: float(np.max(dev[k])) for k in dr.METRICS}
    assert all(v > 0 for v in worst.values()), worst
    return {k: 4 * v for k, v in worst.items()}, worst


def against_float64(got, ref, bnds, where):
    """One set of records (flat, DUMP_DTYPE) against the float64 ones: the integer fields equal on
    every job, every deviation within its bound.  Returns the worst deviation per field."""
    for k in dr.INTS:
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, (where, k, 'jobs', bad[:8], got[k][bad[:8]], ref[k][bad[:8]])
    dev = dr.deviations(got, ref)
    worst = {k: float(np.max(dev[k])) for k in dr.METRICS}
    for k in dr.METRICS:
        assert worst[k] <= bnds[k], (where, k, 'job', int(np.argmax(dev[k])), 'deviation', worst[k],
                                     'bound', bnds[k], 'ratio', worst[k] / bnds[k])
    return worst
