"""trk_corr_kernel<CG, FMT> (csrc/gpsmi_trk_corr.h) against the float64 restatement of the
operation (tests/corr_ref.py), every variant: CG = 1, 2, 4, 6 forced through the options
"corr_small1" / "corr_small2" / "corr_cg" on a live handle, complex64 and raw uint16 input, the
piped fold (CORR_AVG = 8) and the row-at-a-time one, partly filled and partly closed channel
groups, block counts on both sides of the workgroup map's switch.

What the kernel returns per (block, channel) through gpsmi_trk_replay -- mx, epl, corr_mean,
corr_std, norm_max_corr, delay, code_phase, delay_used -- must be
  - byte-identical across CG and input format (the choice of CG depends on the launch size, and
    "replay equals the closed loop, whatever the launch size" is the contract);
  - independent of the neighbours in the channel group;
  - within 4 x the float32 oracle's own worst deviation from float64 over the same jobs (the
    oracle carries a float32 carrier phase, the kernel a double one: a correct kernel has room to
    spare; the factor covers the different rounding order of the LDS FFT).  The bounds are
    computed in the tests from those jobs; DESIGN.md section 4.4 has the figures of an MI355X run.
A job is left out of the mx equality when the two largest float64 lags are within 1e-4 of the
peak, and out of the delay / code_phase comparison when |norm - CORR_MIN| is below the norm bound:
at most 1 % of a test's jobs each, asserted."""
import numpy as np
import pytest

import corr_ref as cr

CORR_MIN = 8.0
VARIANT_GAP = 1e-4                    # top-two gap below which the argmax is not determined
LEFT_OUT_CAP = 0.01

# How CG is forced (the ABI keeps corr_small1 <= corr_small2, hence the order of the settings):
# 'small' through the job-count thresholds, 'option' through "corr_cg" with both thresholds at 0.
BIG = 1 << 24
CG_SETTINGS = {
    (1, 'small'): (('corr_small2', BIG), ('corr_small1', BIG)),
    (2, 'small'): (('corr_small1', 0), ('corr_small2', BIG)),
    (2, 'option'): (('corr_small1', 0), ('corr_small2', 0), ('corr_cg', 2)),
    (4, 'option'): (('corr_small1', 0), ('corr_small2', 0), ('corr_cg', 4)),
    (6, 'option'): (('corr_small1', 0), ('corr_small2', 0), ('corr_cg', 6)),
}
FORMATS = ('c64', 'u8')
VARIANTS = tuple((cg, how, fmt) for (cg, how) in CG_SETTINGS for fmt in FORMATS)

# The variant matrix: (N_CYC, CORR_AVG, channels, blocks); every row runs under every VARIANT.
# CORR_AVG 8 is the piped fold, everything else the row-at-a-time one; first = (N_CYC - n) // 2 is
# 0 where CORR_AVG >= N_CYC (12 is clamped at N_CYC = 8) and non-zero otherwise.  The channel
# counts leave every remainder against CG = 2, 4, 6; 1 .. 7 blocks map linearly, 8 and more
# through the XCD map, 9 and 13 with padding workgroups (gpsmi_wgmap.h).
MATRIX = (
    (32, 8, 12, 64), (32, 1, 1, 13), (32, 4, 2, 9), (32, 5, 13, 8), (32, 12, 7, 7), (32, 32, 3, 1),
    (32, 8, 10, 9),
    (16, 8, 5, 9), (16, 1, 11, 13), (16, 4, 13, 64), (16, 5, 3, 8), (16, 12, 2, 7), (16, 16, 7, 1),
    (8, 8, 11, 64), (8, 1, 5, 7), (8, 4, 12, 1), (8, 5, 1, 8), (8, 12, 13, 9), (8, 8, 7, 13),
)
AXES = {'n_cyc': (32, 16, 8), 'corr_avg': (8, 1, 4, 5, 12, 'N_CYC'),
        'nch': (1, 2, 3, 5, 7, 10, 11, 12, 13), 'nb': (1, 7, 8, 9, 13, 64)}

ABSENT = (1, 33, 35, 37)
# (prn, doppler Hz, delay samples, amplitude): strong and weak, the ends of the frequency range, 0
SATS = ((3, 5000.0, 1462.31, 0.12), (8, -5000.0, 11.77, 0.12), (11, 0.0, 2046.52, 0.09),
        (14, 1234.5, 255.49, 0.09), (19, -2871.3, 1023.98, 0.06), (22, 3980.2, 512.03, 0.06),
        (26, -610.7, 1790.64, 0.045), (30, 2222.2, 767.25, 0.035), (31, -4400.4, 300.5, 0.028))
N_DISTINCT = 8                        # distinct blocks of a scene; longer launches tile them

_SCENES = {}


def _scene_blocks(n_cyc):
    """(complex64 blocks, raw uint16 blocks) of the module's scene at this block length; the
    complex64 block is the decode of the raw one, bit for bit."""
    if n_cyc not in _SCENES:
        from gpsmi import synth
        sc = synth.Scene(sats=[synth.Sat(prn=p, doppler=f, delay=d, amp=a, phase0=0.7 * i)
                               for i, (p, f, d, a) in enumerate(SATS)],
                         seed=4100 + n_cyc, n_cyc=n_cyc)
        raws = [sc.block_raw(b) for b in range(N_DISTINCT)]
        c64 = [synth.raw_to_c64(r) for r in raws]
        for r, x in zip(raws, c64):
            assert cr.decode_u8(r).tobytes() == x.tobytes()
        _SCENES[n_cyc] = (c64, raws)
    return _SCENES[n_cyc]


PHASE_TOP = np.nextafter(np.float32(2 * np.pi), np.float32(0))     # the largest float32 below 2 pi


def _template_row():
    """A state row as gpsmi_trk_open leaves it (every field the later kernels range-check)."""
    from gpsmi.engine import TrkEngine
    eng = TrkEngine(max_ch=1)
    eng.open(0, 3, 0.0, 0)
    row = eng.get_state(0).copy()
    eng.close()
    return row


def _draw_table(rng, nb, nch, template):
    """State table and forced delays of nb x nch jobs from a seeded generator: PRNs present (at
    their Doppler, or far off it) and absent; FREQ over +-5000, 0 and between, as a float32
    (omega0 = 0) or as the Python float the loop starts with (omega0 = float32(2 pi FREQ)); PHASE
    in [0, 2 pi) with exactly 0 and the largest float32 below 2 pi; DELAY anywhere; forced delays
    a mix of -1 and values >= 0."""
    from gpsmi.engine import STATE_DTYPE
    assert 2 * np.pi - 1e-6 < float(PHASE_TOP) < 2 * np.pi
    table = np.empty((nb, nch), dtype=STATE_DTYPE)
    table[...] = template
    forced = np.full((nb, nch), -1, dtype=np.int32)
    for j in range(nb * nch):
        i, c = divmod(j, nch)
        kind = int(rng.integers(0, 10))
        if kind < 6:                                   # a satellite of the scene, near its Doppler
            prn, dop = SATS[int(rng.integers(0, len(SATS)))][:2]
            f = float(np.clip(dop + rng.uniform(-12, 12), -5000.0, 5000.0)) if kind else dop
        elif kind < 8:                                 # a PRN that is not there
            prn = ABSENT[int(rng.integers(0, len(ABSENT)))]
            f = (-5000.0, 5000.0, 0.0, float(rng.uniform(-5000, 5000)))[int(rng.integers(0, 4))]
        else:                                          # a satellite of the scene, off its Doppler
            prn = SATS[int(rng.integers(0, len(SATS)))][0]
            f = float(rng.uniform(-5000, 5000))
        st = table[i, c]
        st['prn'] = prn
        st['freq'] = np.float32(f)
        st['omega0'] = np.float32(2 * np.pi * f) if rng.integers(0, 2) else np.float32(0)
        st['phase'] = (np.float32(0), PHASE_TOP, np.float32(rng.uniform(0, 6.28)),
                       np.float32(rng.uniform(0, 6.28)))[j % 4]
        st['delay'] = (0, 2047, int(rng.integers(0, 2048)))[min(j % 5, 2)]
        table[i, c] = st
        if rng.integers(0, 2):
            forced[i, c] = (0, 2047, int(rng.integers(0, 2048)))[min(int(rng.integers(0, 6)), 2)]
    return table, forced


def _references(blocks, rows, table, forced, n_cyc, corr_avg):
    """(float64 records, oracle records) [nb, nch] of a table; rows[i] = the block of table row i."""
    nb, nch = table.shape
    ref = np.zeros((nb, nch), cr.CORR_DTYPE)
    orc = np.zeros((nb, nch), cr.CORR_DTYPE)
    for i in range(nb):
        for c in range(nch):
            if table[i, c]['prn'] > 0:
                args = (blocks[rows[i]], table[i, c], n_cyc, corr_avg, CORR_MIN, int(forced[i, c]))
                ref[i, c] = cr.corr_ref(*args)
                orc[i, c] = cr.oracle_record(*args)
    return ref, orc


def _bounds(orc, ref):
    """Per field 4 x the oracle's worst deviation from float64 over the jobs given (flat arrays),
    with the figures themselves."""
    ok = (orc['mx'] == ref['mx']) & ((orc['delay'] >= 0) == (ref['delay'] >= 0))
    assert ok.mean() >= 1 - 2 * LEFT_OUT_CAP
    dev = cr.deviations(orc, ref)
    worst = {k: float(np.max(dev[k][ok])) for k in cr.METRICS}
    assert all(v > 0 for v in worst.values()), worst
    return {k: 4 * v for k, v in worst.items()}, worst


def _against_float64(recs, ref, forced, bounds, where):
    """One set of kernel records (flat) against the float64 ones.  Returns the kernel's worst
    deviation per field and the two left-out counts."""
    n = ref.size
    mx_open = ref['gap'] < VARIANT_GAP
    br_open = ref['margin'] < bounds['norm_max_corr'] * np.abs(ref['norm_max_corr'])
    assert mx_open.sum() <= LEFT_OUT_CAP * n, (where, 'argmax left out', int(mx_open.sum()), n)
    assert br_open.sum() <= LEFT_OUT_CAP * n, (where, 'CORR_MIN branch left out', int(br_open.sum()), n)
    same = recs['mx'] == ref['mx']
    bad = np.flatnonzero(~same & ~mx_open)
    assert bad.size == 0, (where, 'mx', bad[:8], recs['mx'][bad[:8]], ref['mx'][bad[:8]])
    dev = cr.deviations(recs, ref)
    worst = {}
    for k in cr.METRICS:
        use = same if k in ('epl', 'code_phase') else np.ones(n, bool)
        if k == 'code_phase':
            use = use & ~br_open
        worst[k] = float(np.max(dev[k][use]))
        j = int(np.argmax(np.where(use, dev[k], -1.0)))
        assert worst[k] <= bounds[k], (where, k, 'job', j, 'deviation', worst[k], 'bound', bounds[k])
    det = same & ~br_open
    for k in ('delay', 'delay_used'):
        bad = np.flatnonzero(det & (recs[k] != ref[k]))
        assert bad.size == 0, (where, k, bad[:8], recs[k][bad[:8]], ref[k][bad[:8]])
    lost = det & (ref['delay'] < 0)
    assert (recs['code_phase'][lost] == -1.0).all(), (where, 'code_phase below CORR_MIN')
    f = forced >= 0
    assert (recs['delay_used'][f] == forced[f]).all(), (where, 'forced delay')
    return worst, int(mx_open.sum()), int(br_open.sum())


def _force_cg(eng, cg, how):
    for key, value in CG_SETTINGS[cg, how]:
        eng.set_option(key, value)
        assert eng.get_option(key) == value, (key, value)
    s1, s2 = eng.get_option('corr_small1'), eng.get_option('corr_small2')
    return 1 if s1 == BIG else 2 if s2 == BIG else eng.get_option('corr_cg')


def _same_fields(a, b):
    """The eight correlation fields of two record arrays, bytewise: the names that differ."""
    return [k for k in cr.FIELDS if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]


def _replay_variants(n_cyc, corr_avg, blocks, raws, rows, table, forced, variants=VARIANTS):
    """The same IQ and table through every variant on one handle: {variant: records [nb, nch]}."""
    from gpsmi.engine import Config, DeviceBuffer, TrkEngine
    nb, nch = table.shape
    eng = TrkEngine(Config(n_cyc=n_cyc, corr_avg=corr_avg, corr_min=CORR_MIN), max_ch=nch)
    bufs = {}
    out = {}
    try:
        for fmt, src in (('c64', blocks), ('u8', raws)):
            if any(v[2] == fmt for v in variants):
                bufs[fmt] = DeviceBuffer(nb * src[0].nbytes)
                for i in range(nb):
                    bufs[fmt].upload(src[rows[i]], i * src[0].nbytes)
        for cg, how, fmt in variants:
            assert _force_cg(eng, cg, how) == cg
            eng.set_input_format(fmt == 'u8')
            out[cg, how, fmt] = eng.replay(bufs[fmt].ptr, nb, table, forced)
    finally:
        for b in bufs.values():
            b.free()
        eng.close()
    return out


def _report(title, orc_worst, worst, n, n_mx, n_br):
    print(f'\n{title}: {n} jobs, left out {n_mx} (argmax) {n_br} (CORR_MIN branch)')
    print(f'    {"field":<14} {"oracle vs f64":>14} {"kernel vs f64":>14}')
    for k in cr.METRICS:
        print(f'    {k:<14} {orc_worst[k]:>14.2e} {worst[k]:>14.2e}')


def test_matrix_covers_every_axis_value_under_every_variant():
    """Every value of every axis meets every CG and both input formats at least once (counted over
    the case list: a row of MATRIX runs under every VARIANT)."""
    cases = [(n_cyc, 'N_CYC' if ca == n_cyc else ca, nch, nb, cg, fmt)
             for (n_cyc, ca, nch, nb) in MATRIX for (cg, _, fmt) in VARIANTS]
    extra = [(n_cyc, ca, nch, nb, cg, fmt)                 # CORR_AVG 8 at N_CYC 8 is both 8 and N_CYC
             for (n_cyc, ca, nch, nb, cg, fmt) in cases if ca == 'N_CYC' and n_cyc == 8]
    cases += [(n_cyc, 8, nch, nb, cg, fmt) for (n_cyc, ca, nch, nb, cg, fmt) in extra]
    for axis, pos in (('n_cyc', 0), ('corr_avg', 1), ('nch', 2), ('nb', 3)):
        for value in AXES[axis]:
            for cg in (1, 2, 4, 6):
                for fmt in FORMATS:
                    n = sum(1 for c in cases if c[pos] == value and c[4] == cg and c[5] == fmt)
                    assert n >= 1, (axis, value, cg, fmt)
    assert {(cg, how) for cg, how, _ in VARIANTS} == set(CG_SETTINGS)
    for n_cyc, ca, nch, nb in MATRIX:                      # both kinds of `first`, both folds
        assert ca >= 1 and nch >= 1 and nb >= 1
    firsts = {(n_cyc - min(ca, n_cyc)) // 2 == 0 for n_cyc, ca, _, _ in MATRIX}
    assert firsts == {True, False}
    for cg in (2, 4, 6):                                   # every remainder of nch against CG
        assert {nch % cg for _, _, nch, _ in MATRIX} == set(range(cg)), cg


@pytest.mark.gpu
@pytest.mark.parametrize('n_cyc', [32, 16, 8])
def test_variant_matrix_bytewise_and_against_float64(n_cyc):
    """(a) + (c): every row of MATRIX at this block length through every VARIANT.  The eight
    fields are byte-identical across CG and input format, and every variant's records are within
    4 x the oracle's deviation from float64 (bounds over all jobs of the block length)."""
    template = _template_row()
    blocks, raws = _scene_blocks(n_cyc)
    shapes = [m for m in MATRIX if m[0] == n_cyc]
    runs, refs, orcs, forceds = [], [], [], []
    ran = {v: 0 for v in VARIANTS}
    differ = []
    for (_, corr_avg, nch, nb) in shapes:
        rng = np.random.default_rng([n_cyc, corr_avg, nch, nb])
        table, forced = _draw_table(rng, nb, nch, template)
        rows = np.arange(nb) % N_DISTINCT
        out = _replay_variants(n_cyc, corr_avg, blocks, raws, rows, table, forced)
        base = out[VARIANTS[0]]
        assert (base['prn'] == table['prn']).all()
        for v in VARIANTS:
            ran[v] += 1
            names = _same_fields(out[v], base)
            if names:
                differ.append(((n_cyc, corr_avg, nch, nb), v, names))
        ref, orc = _references(blocks, rows, table, forced, n_cyc, corr_avg)
        runs.append(out)
        refs.append(ref.ravel())
        orcs.append(orc.ravel())
        forceds.append(forced.ravel())
    assert all(n == len(shapes) for n in ran.values()), ran
    ref, orc, forced = np.concatenate(refs), np.concatenate(orcs), np.concatenate(forceds)
    found = ref['delay'] >= 0
    assert found.any() and not found.all()                 # both sides of CORR_MIN
    bounds, orc_worst = _bounds(orc, ref)
    worst = dict.fromkeys(cr.METRICS, 0.0)
    for v in VARIANTS:
        recs = np.concatenate([out[v].ravel() for out in runs])
        w, n_mx, n_br = _against_float64(recs, ref, forced, bounds, (n_cyc, v))
        worst = {k: max(worst[k], w[k]) for k in worst}
    _report(f'variant matrix, N_CYC {n_cyc}, {len(shapes)} shapes x {len(VARIANTS)} variants',
            orc_worst, worst, ref.size, n_mx, n_br)
    print(f'    found {int(found.sum())}, below CORR_MIN {int((~found).sum())}')
    assert not differ, differ


@pytest.mark.gpu
def test_channel_order_and_solo_channels():
    """(b): permuting the channel order of a table permutes the records and changes nothing else;
    a channel's record is the same alone (one channel per block) as inside a full group.  Under
    every CG; the records against float64 as well."""
    n_cyc, corr_avg, nch, nb = 32, 8, 12, 9
    blocks, raws = _scene_blocks(n_cyc)
    table, forced = _draw_table(np.random.default_rng(77), nb, nch, _template_row())
    rows = np.arange(nb) % N_DISTINCT
    perm = np.array([7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 6, 4])
    assert sorted(perm) == list(range(nch))
    variants = [v for v in VARIANTS if v[2] == 'c64'] + [(4, 'option', 'u8')]
    out = _replay_variants(n_cyc, corr_avg, blocks, raws, rows, table, forced, variants)
    outp = _replay_variants(n_cyc, corr_avg, blocks, raws, rows, np.ascontiguousarray(table[:, perm]),
                            np.ascontiguousarray(forced[:, perm]), variants)
    base = out[variants[0]]
    for v in variants:
        assert not _same_fields(out[v], base), v
        assert not _same_fields(outp[v], base[:, perm]), ('permuted', v)
        assert (outp[v]['prn'] == table['prn'][:, perm]).all()
    for c in (0, 5, 11):
        solo = _replay_variants(n_cyc, corr_avg, blocks, raws, rows, np.ascontiguousarray(table[:, c:c + 1]),
                                np.ascontiguousarray(forced[:, c:c + 1]),
                                [(1, 'small', 'c64'), (4, 'option', 'c64'), (6, 'option', 'u8')])
        for v, rec in solo.items():
            assert not _same_fields(rec[:, 0], base[:, c]), ('alone', c, v)
    ref, orc = _references(blocks, rows, table, forced, n_cyc, corr_avg)
    bounds, orc_worst = _bounds(orc.ravel(), ref.ravel())
    worst, n_mx, n_br = _against_float64(base.ravel(), ref.ravel(), forced.ravel(), bounds, 'channel order')
    _report('channel order and solo channels', orc_worst, worst, ref.size, n_mx, n_br)


# closed slots of 13 channels, one pattern per receiver: nothing; the first slot of every group; a
# slot that is the last of a CG = 2 group and a middle one at CG = 4 and 6; the last of the first
# CG = 4 group; the last of the first CG = 6 group; a whole CG = 4 group; a whole CG = 6 group; the
# second CG = 6 group; the lone channel of the last group; all but one; a scatter; the last CG = 4
# group and the lone channel
CLOSED = ((), (0,), (1,), (3,), (5,), (0, 1, 2, 3), (0, 1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 11), (12,),
          (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12), (2, 4, 9, 11), (8, 9, 10, 11, 12))


@pytest.mark.gpu
def test_closed_channels_leave_their_neighbours_alone():
    """(b), closed channels: batched receivers (gpsmi_trk_set_streams) that all get the same block
    and the same 13 state rows, each with its own pattern of closed channels.  An open channel's
    record is the record of the receiver with nothing closed, byte for byte; closed channels return
    prn = 0 and n_dumps = 0.  Under every CG and both input formats; against float64 as well."""
    from gpsmi.engine import Config, DeviceBuffer, TrkEngine
    n_cyc, corr_avg, nch = 32, 8, 13
    R = len(CLOSED)
    blocks, raws = _scene_blocks(n_cyc)
    table, _ = _draw_table(np.random.default_rng(1313), 1, nch, _template_row())
    forced = np.full((1, nch), -1, np.int32)               # the closed loop has no forced delay
    eng = TrkEngine(Config(n_cyc=n_cyc, corr_avg=corr_avg, corr_min=CORR_MIN), max_ch=nch, streams=R)
    bufs = {'c64': DeviceBuffer(R * blocks[3].nbytes), 'u8': DeviceBuffer(R * raws[3].nbytes)}
    bufs['c64'].upload(np.stack([blocks[3]] * R))
    bufs['u8'].upload(np.stack([raws[3]] * R))
    outs = {}
    try:
        for cg, how, fmt in VARIANTS:
            assert _force_cg(eng, cg, how) == cg
            eng.set_input_format(fmt == 'u8')
            for r in range(R):                             # the step before advanced the states
                for c in range(nch):
                    if c not in CLOSED[r]:                 # (the others were never opened)
                        eng.set_state(c, table[0, c], stream=r)
            outs[cg, how, fmt] = eng.process(bufs[fmt].ptr).reshape(R, nch)
    finally:
        for b in bufs.values():
            b.free()
        eng.close()
    base = outs[VARIANTS[0]][0]
    assert (base['prn'] == table['prn'][0]).all()
    for v, out in outs.items():
        assert not _same_fields(out[0], base), v
        for r in range(R):
            for c in range(nch):
                if c in CLOSED[r]:
                    assert out[r, c]['prn'] == 0 and out[r, c]['n_dumps'] == 0, (v, r, c)
                else:
                    assert out[r, c].tobytes() == out[0, c].tobytes(), (v, r, c)
    # 13 jobs are too few for a bound of their own: the oracle's deviations over the table of the
    # channel-order test (same scene, block length and CORR_AVG, 108 jobs) join them
    t2, f2 = _draw_table(np.random.default_rng(77), 9, 12, _template_row())
    rows2 = np.arange(9) % N_DISTINCT
    ref2, orc2 = _references(blocks, rows2, t2, f2, n_cyc, corr_avg)
    ref, orc = _references(blocks, [3], table, forced, n_cyc, corr_avg)
    bounds, orc_worst = _bounds(np.concatenate([orc.ravel(), orc2.ravel()]),
                                np.concatenate([ref.ravel(), ref2.ravel()]))
    # (1 % of 13 jobs is none: a job left out here fails the test)
    worst, n_mx, n_br = _against_float64(base, ref.ravel(), forced.ravel(), bounds, 'closed channels')
    _report('closed channels', orc_worst, worst, ref.size, n_mx, n_br)


# the circular wrap (0, 2047), lag = t + 256 r: the first and last thread of a register row (255,
# 256), of a wave (1023 / 1024 in row 3, 511 / 512 in row 1 / 2) and their neighbours
PEAK_LAGS = (0, 1, 2, 254, 255, 256, 257, 511, 512, 1023, 1024, 1025, 2045, 2046, 2047)
PEAK_SATS = ((2, -5000.0), (5, -3100.5), (9, -800.25), (13, 420.0), (17, 1999.75), (23, 3777.0), (29, 5000.0))


def _peak_blocks(n_cyc):
    """One block per entry of PEAK_LAGS: seven satellites, each its replica rolled to a chosen lag
    (the same roll in every period) with a weaker copy one lag further on alternating sides, so
    that the neighbours of the peak differ; a carrier per satellite and weak noise.  Returns the
    blocks and lag[b, c]."""
    from gpsmi import codes
    rng = np.random.default_rng(2047)
    n = n_cyc * cr.CS
    t = (np.arange(n, dtype=np.float64) + 1.0) / cr.FS
    nl = len(PEAK_LAGS)
    lags = np.array([[PEAK_LAGS[(b + 2 * c) % nl] for c in range(len(PEAK_SATS))] for b in range(nl)])
    blocks = []
    for b in range(nl):
        x = 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))
        for c, (prn, f) in enumerate(PEAK_SATS):
            rep = codes.code_replica(prn, cr.CS)
            side = 1 if c % 2 else -1
            one = 0.07 * np.roll(rep, lags[b, c]) + 0.03 * np.roll(rep, lags[b, c] + side)
            x = x + np.tile(one, n_cyc) * np.exp(1j * (0.4 * c + 2 * np.pi * f * t))
        blocks.append(x.astype(np.complex64))
    return blocks, lags


@pytest.mark.gpu
def test_peak_at_every_boundary():
    """(d): the true peak on each lag of PEAK_LAGS -- the circular wrap and the seams of
    corr_stats8 (thread, wave and register-row boundaries of lag = t + 256 r) -- in every channel
    position of a group; mx, both neighbours and code_phase against float64 under CG 1, 4 and 6."""
    n_cyc, corr_avg = 32, 8
    blocks, lags = _peak_blocks(n_cyc)
    nb, nch = lags.shape
    template = _template_row()
    from gpsmi.engine import STATE_DTYPE
    table = np.empty((nb, nch), dtype=STATE_DTYPE)
    table[...] = template
    rng = np.random.default_rng(15)
    for c, (prn, f) in enumerate(PEAK_SATS):
        table['prn'][:, c] = prn
        table['freq'][:, c] = np.float32(f)
    table['phase'] = rng.uniform(0, 6.28, (nb, nch)).astype(np.float32)
    table['delay'] = rng.integers(0, 2048, (nb, nch))
    forced = np.full((nb, nch), -1, np.int32)
    rows = np.arange(nb)
    ref, orc = _references(blocks, rows, table, forced, n_cyc, corr_avg)
    assert (ref['mx'] == lags).all() and (ref['delay'] == lags).all()      # every peak where it was put
    assert set(ref['mx'].ravel()) == set(PEAK_LAGS)
    assert ref['gap'].min() > 0.1
    bounds, orc_worst = _bounds(orc.ravel(), ref.ravel())
    variants = [(1, 'small', 'c64'), (2, 'small', 'c64'), (4, 'option', 'c64'), (6, 'option', 'c64')]
    out = _replay_variants(n_cyc, corr_avg, blocks, None, rows, table, forced, variants)
    worst = dict.fromkeys(cr.METRICS, 0.0)
    for v in variants:
        assert (out[v]['mx'] == lags).all(), v
        w, n_mx, n_br = _against_float64(out[v].ravel(), ref.ravel(), forced.ravel(), bounds, ('peaks', v))
        assert n_mx == 0 and n_br == 0
        worst = {k: max(worst[k], w[k]) for k in worst}
        assert not _same_fields(out[v], out[variants[0]]), v
    _report('peak at every boundary', orc_worst, worst, ref.size, 0, 0)
