"""Every correlation path of acquisition (csrc/gpsmi_acq.hip: acq_direct_chunk and the 2048 kernels
of gpsmi_acq_search.h) against the float64 restatement of the operation (tests/acq_ref.py): the
2048-point FFT kernels (G = 1 and G = 4 spectrum, MODE 0 / 1 / 2 correlation), the native 16368
correlation, the zero-padded 32768-point pair and the time-domain kernel, each at the code lengths
where its indexing changes (acq_ref.MATRIX), always through search_ex / search_noncoherent(nbr=True)
/ search_deep(nbr=True) so that the neighbours of the peak are compared too.

Per test, over its cells:
  - argmax equals the float64 one wherever the two largest float64 lags are more than 1e-4 apart;
    elsewhere it must be a lag within 1e-4 of the peak, and lo / hi are held to the reference's
    neighbours of that lag.  Such cells: none in a test of fewer than 100 cells, 1 % otherwise,
    asserted (test_acq_ref.py holds the seeded inputs to it without a GPU).
  - peak, lo, hi, mean as |value - ref| / rms and std relatively are within
      2048 and native 16368: 4 x the float32 oracle's own worst deviation over the same cells (the
        factor is test_gpu_trk_corr.py's: the same arithmetic in another rounding order).  The
        oracle is given the replica as the handle is, in single precision, so that its product,
        inverse transform, |.|, segment sums and statistics are float32 like the kernels'.  Fed
        fft_cacode's complex128 spectrum, as acq_table feeds it, only its wipe-off and forward
        transform are float32; an MI355X run against that tighter figure had the kernels at up to
        1.2 x (2048) and 2.8 x (16368, std: pfa_corr_kernel's segmented modes take the variance
        from the sum of squares) of 4 x its deviation -- float32 rounding behind the forward
        transform, which that oracle does not have, and no defect: DESIGN.md 4.2 has both tables;
      32768 pair: 4 x that of the oracle with a zero-padded 32768-point float32 transform pair;
      time domain: peak, lo, hi within acq_ref.direct_bound at their lag.  From it, mean within the
        bound's mean over the lags plus 2 (L / 256 + 16) 2^-24 of the mean (corr_stats_kernel's
        strided sums of L / 256 terms and its 16-way tree, positive terms), std within the bound's
        rms (the population std of a perturbed surface moves by at most the perturbation's rms)
        plus twice that relative term.
  - integer-valued inputs at 0 Hz make every accumulator of acq_fold_kernel and
    circ_corr_direct_kernel exact in float32: there peak, lo, hi are within 2 float32 ulp of the
    exact surface (two squares, their sum, the root: half an ulp each before the root), argmax is
    exact including on an exact tie, mean within 2 (L / 256 + 16) 2^-24 and std within twice that.
The figures of an MI355X run (kernel error over bound per row) are in DESIGN.md 4.2."""
import numpy as np
import pytest

import acq_ref as ar

pytestmark = pytest.mark.gpu

FACTOR = 4
ULPS = 2


def _engine(cs, n_cyc, codephase, prns=ar.PRNS, reps=None):
    """A handle on the path `codephase` forces (0: the length's own), with the test's replicas."""
    from gpsmi.engine import AcqEngine, Config, check, clear_default, ptr, set_default
    if codephase:
        set_default('codephase', codephase)
    try:
        e = AcqEngine(Config(code_samples=cs, n_cyc=n_cyc), prns=prns)
    finally:
        if codephase:
            clear_default('codephase')
    if reps is not None:
        for p in prns:
            r = np.ascontiguousarray(reps[p], np.float32)
            assert r.shape == (cs,)
            check(e.lib.gpsmi_acq_set_replica_time(e.h, int(p), ptr(r)), 'gpsmi_acq_set_replica_time')
    return e


def _records(tab, nbr):
    got = np.zeros(tab.shape, ar.REC_DTYPE)
    for k in ('argmax', 'peak', 'mean', 'std'):
        got[k] = tab[k]
    got['lo'], got['hi'] = nbr[..., 0], nbr[..., 1]
    for k in ar.FIELDS:
        assert np.isfinite(got[k]).all(), k
    return got


def _search(e, iq, name, search):
    prns, freqs, n_coh, n_seg, _, carrier = ar.case_search(name, search)
    if search[0] == 'coh':
        return _records(*e.search_ex(iq, prns, freqs, n_coh))
    if search[0] == 'nc':
        return _records(*e.search_noncoherent(iq, prns, freqs, n_coh, n_seg, nbr=True))
    return _records(*e.search_deep(iq, prns, freqs, n_coh, n_seg, f_offset=0.0, carrier_hz=carrier, nbr=True))


def _settle_argmax(got, ref, surfaces, where):
    """The argmax rule.  Returns (the reference with lo / hi of an excused cell taken at the
    kernel's argmax, the number of excused cells)."""
    ref = ref.copy()
    excused = 0
    for idx in np.ndindex(ref.shape):
        if ref[idx]['gap'] > ar.NEAR_TIE:
            assert got[idx]['argmax'] == ref[idx]['argmax'], (where, idx, got[idx], ref[idx])
            continue
        S, am = surfaces[idx], int(got[idx]['argmax'])
        assert 0 <= am < len(S) and S[am] >= S.max() * (1 - ar.NEAR_TIE), (where, idx, am, ref[idx])
        ref[idx]['lo'], ref[idx]['hi'] = S[(am - 1) % len(S)], S[(am + 1) % len(S)]
        excused += 1
    return ref, excused


def _worst(dev, use=None):
    return {k: float(np.max(dev[k] if use is None or k in ('mean', 'std') else np.where(use, dev[k], 0.0)))
            for k in ar.METRICS}


def _report(title, cells, excused, rows):
    print(f'\n{title}: {cells} cells, {excused} excused')
    print(f'    {"field":<6} {"kernel":>10} {"bound":>10} {"ratio":>7}')
    for k, err, bound in rows:
        print(f'    {k:<6} {err:>10.3e} {bound:>10.3e} {err / bound:>7.3f}')


def _hold_to_oracle(title, gots, refs, orcs, excused):
    """Flat records of a test: the kernel's deviations within FACTOR x the oracle's worst."""
    got, ref, orc = (np.concatenate([a.ravel() for a in x]) for x in (gots, refs, orcs))
    assert excused <= ar.excused_cap(ref.size), (title, 'near ties', excused, ref.size)
    same = orc['argmax'] == ref['argmax']
    assert same.mean() >= 0.98, (title, 'the oracle itself leaves the float64 argmax')
    o_worst = _worst(ar.deviations(orc, ref), same)
    assert all(v > 0 for v in o_worst.values()), o_worst
    dev = ar.deviations(got, ref)
    worst = _worst(dev)
    _report(title, ref.size, excused, [(k, worst[k], FACTOR * o_worst[k]) for k in ar.METRICS])
    for k in ar.METRICS:
        j = int(np.argmax(dev[k]))
        assert worst[k] <= FACTOR * o_worst[k], (title, k, 'cell', j, got[j], ref[j], worst[k], FACTOR * o_worst[k])


def _stats_term(L):
    return 2 * (L / 256 + 16) * 2.0 ** -24


def _hold_to_direct_bound(title, name, search, which, got, ref, rows):
    """One time-domain search against acq_ref.direct_bound, cell by cell; appends the worst
    error-over-bound per field to rows."""
    cs = ar.MATRIX[name][1]
    prns, freqs, n_coh = ar.case_search(name, search)[:3]
    iq = ar.case_inputs(name)[which][0]
    ratio = {k: 0.0 for k in ar.METRICS}
    for b, f in enumerate(freqs):
        for j, p in enumerate(prns):
            B = ar.direct_bound(iq, f, p, cs, n_coh)
            g, r = got[b, j], ref[b, j]
            am = int(g['argmax'])
            bound = {'peak': B[am], 'lo': B[(am - 1) % cs], 'hi': B[(am + 1) % cs],
                     'mean': np.mean(B) + _stats_term(cs) * r['mean'],
                     'std': np.sqrt(np.mean(B * B)) + 2 * _stats_term(cs) * r['std']}
            for k in ar.METRICS:
                err = abs(float(g[k]) - r[k])
                assert err <= bound[k], (title, search, k, 'bin', f, 'prn', p, g, r, err, bound[k])
                ratio[k] = max(ratio[k], err / bound[k])
    rows.append((search, which, ratio))


@pytest.mark.parametrize('name', list(ar.MATRIX))
def test_matrix_row_against_float64(name):
    path, cs, codephase, searches = ar.MATRIX[name]
    n_cyc = ar.case_periods(name)[0]
    prns = ar.case_search(name, searches[0])[0]
    e = _engine(cs, n_cyc, codephase, prns)
    gots, refs, orcs, ratios, excused = [], [], [], [], 0
    try:
        for search in searches:
            for which, (iq, _) in enumerate(ar.case_inputs(name)):
                got = _search(e, iq, name, search)
                ref, surfaces = ar.case_reference(name, search, which)
                ref, n = _settle_argmax(got, ref, surfaces, (name, search, which))
                excused += n
                gots.append(got)
                refs.append(ref)
                if path == 'direct':
                    _hold_to_direct_bound(name, name, search, which, got, ref, ratios)
                    continue
                cprns, freqs, n_coh, n_seg, shifts, _ = ar.case_search(name, search)
                oracle = ar.oracle_record_padded if path == 'big' else ar.oracle_record
                orcs.append(oracle(iq, freqs, cprns, cs, n_coh, n_seg, shifts))
    finally:
        e.close()
    if path != 'direct':
        _hold_to_oracle(name, gots, refs, orcs, excused)
        return
    cells = sum(r.size for r in refs)
    assert excused <= ar.excused_cap(cells), (name, 'near ties', excused, cells)
    print(f'\n{name}: {cells} cells, {excused} excused; worst error over acq_ref.direct_bound')
    for search, which, ratio in ratios:
        print(f'    {search} input {which}: ' + ' '.join(f'{k} {ratio[k]:.1e}' for k in ar.METRICS))


ZERO_CASES = [
    ('fft2048', 2048, 0, (('coh', 1), ('coh', 3), ('coh', 4), ('coh', 5), ('nc', 1, 2), ('nc', 2, 2),
                          ('deep', 1, 2), ('deep', 2, 2))),
    ('pfa', 16368, 0, (('coh', 1), ('coh', 2), ('nc', 2, 2), ('deep', 2, 2))),
    ('big', 1040, 0, (('coh', 1), ('coh', 2))),
    ('big', 16384, 0, (('coh', 1),)),
    ('direct', 1040, 1, (('coh', 1), ('coh', 2))),
    ('direct', 16400, 0, (('coh', 1),)),
]


@pytest.mark.parametrize('path, cs, codephase, searches', ZERO_CASES, ids=[f'{c[0]}{c[1]}' for c in ZERO_CASES])
def test_all_zero_input_gives_the_zero_record(path, cs, codephase, searches):
    """The all-equal surface, the first-index rule's only exact case: argmax 0 and peak, mean, std,
    lo, hi exactly 0 -- no NaN from a 0 / 0 or a root of a negative rounding -- on all four paths
    and in MODE 1 / 2.  (No raw byte decodes to exactly 0: complex64 input only.)"""
    iq = np.zeros(5 * cs, np.complex64)
    prns, freqs = [1, 20, 37], [-5000.0, 0.0, 1250.0]
    e = _engine(cs, 5, codephase, prns)
    try:
        for search in searches:
            n_coh, n_seg = search[1], (search[2] if len(search) > 2 else 1)
            if search[0] == 'coh':
                tab, nbr = e.search_ex(iq, prns, freqs, n_coh)
            elif search[0] == 'nc':
                tab, nbr = e.search_noncoherent(iq, prns, freqs, n_coh, n_seg, nbr=True)
            else:
                carrier = n_coh * cs / ar.DEEP_K[cs]
                assert ar.deep_shifts(freqs, n_coh, n_seg, cs, carrier)[:, 1].any()
                tab, nbr = e.search_deep(iq, prns, freqs, n_coh, n_seg, carrier_hz=carrier, nbr=True)
            assert tab.tobytes() == np.zeros_like(tab).tobytes(), (search, tab)
            assert nbr.tobytes() == np.zeros_like(nbr).tobytes(), (search, nbr)
    finally:
        e.close()


def _ulps(got, ref):
    """|got - ref| in float32 ulps of ref."""
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def _exact_records(iq, prns, cs, n_avg, reps):
    ref = np.zeros((1, len(prns)), ar.REC_DTYPE)
    for j, p in enumerate(prns):
        ref[0, j] = ar.exact_integer_record(iq, p, cs, n_avg, reps)
    return ref


def _hold_to_exact(where, got, ref, cs, worst):
    assert np.array_equal(got['argmax'], ref['argmax']), (where, got['argmax'], ref['argmax'])
    for k in ('peak', 'lo', 'hi'):
        u = _ulps(got[k], ref[k])
        worst[k] = max(worst.get(k, 0.0), float(u.max()))
        assert (u <= ULPS).all(), (where, k, got[k], ref[k], u)
    for k, bound in (('mean', _stats_term(cs)), ('std', 2 * _stats_term(cs))):
        rel = np.abs(got[k] - ref[k]) / ref[k]
        worst[k] = max(worst.get(k, 0.0), float(rel.max() / bound))
        assert (rel <= bound).all(), (where, k, got[k], ref[k], rel, bound)


@pytest.mark.parametrize('name', list(ar.INTEGER_DIRECT))
def test_time_domain_path_is_exact_on_integer_input(name):
    """Section "integer-valued inputs" of the module docstring, at every time-domain length of the
    matrix: +-1 replicas through gpsmi_acq_set_replica_time, samples from -3 .. 3 plus a roll(rep, d)
    with peaks at 0, cs - 1, both sides of the first lag tile's end and mid-tile, n_avg 1, 2, 4
    (1 / n_avg a power of two), the bin 0 Hz; then the same replica at two rolls, an exact tie."""
    cs, codephase = ar.INTEGER_DIRECT[name]
    reps, iq, sats, n_avgs = ar.integer_case(cs)
    prns = list(ar.PRNS)
    e = _engine(cs, max(n_avgs), codephase, prns, reps)
    worst = {}
    try:
        for n_avg in n_avgs:
            got = _records(*e.search_ex(iq, prns, [0.0], n_avg))
            ref = _exact_records(iq, prns, cs, n_avg, reps)
            for prn, _, lag, a in sats:
                assert ref['argmax'][0, prns.index(prn)] == lag
            _hold_to_exact((name, n_avg), got, ref, cs, worst)
        hi, lo = ar.tie_lags(cs)
        x = ar.tie_input(cs, 1, reps, 20, (hi, lo))
        got = _records(*e.search_ex(x, [20], [0.0], 1))
        ref, S = ar.exact_integer_record(x, 20, cs, 1, reps, surface=True)
        assert S[lo] == S[hi] == S.max() and ref['argmax'] == lo < hi
        _hold_to_exact((name, 'tie'), got, ref.reshape(1, 1), cs, worst)
    finally:
        e.close()
    print(f'\n{name} integer-exact: ulps ' + ' '.join(f'{k} {worst[k]:.2f}' for k in ('peak', 'lo', 'hi'))
          + f'; mean {worst["mean"]:.3f} std {worst["std"]:.3f} of their bounds')


@pytest.mark.parametrize('cs', ar.INTEGER_BIG)
def test_integer_input_through_the_32768_pair(cs):
    """The same integer inputs put peaks on the 32768-pair path's own boundaries (L % 256 = 16, and
    N - L = L): against float64 under that path's oracle-derived bound."""
    reps, iq, _, n_avgs = ar.integer_case(cs)
    prns = list(ar.PRNS)
    e = _engine(cs, max(n_avgs), 0, prns, reps)
    gots, refs, orcs, excused = [], [], [], 0
    try:
        for n_avg in n_avgs:
            got = _records(*e.search_ex(iq, prns, [0.0], n_avg))
            surf = {}
            ref = ar.acq_ref(iq, [0.0], prns, cs, n_avg, reps=reps, surfaces=surf)
            ref, n = _settle_argmax(got, ref, surf, (cs, n_avg))
            excused += n
            gots.append(got)
            refs.append(ref)
            orcs.append(ar.oracle_record_padded(iq, [0.0], prns, cs, n_avg, reps=reps))
    finally:
        e.close()
    _hold_to_oracle(f'integer input, 32768 pair at {cs}', gots, refs, orcs, excused)


def test_second_chunk_of_the_32768_pair():
    """37 PRNs x 14 bins = 518 cells at 1024 samples, above the 512 cells of a chunk of
    big_corr_launch: cells 512 .. 517 (the last bin, PRNs 32 .. 37) against float64, and the last
    bin's 37 records byte for byte those of the same bin searched in a call (one chunk) of its own."""
    cs, prns, bins = ar.CHUNK_CS, list(ar.CHUNK_PRNS), list(ar.CHUNK_BINS)
    assert len(prns) * len(bins) == 518 and 512 // len(prns) == len(bins) - 1
    iq = ar.chunk_input()
    e = _engine(cs, 1, 0, prns)
    try:
        tab, nbr = e.search_ex(iq, prns, bins, 1)
        tab1, nbr1 = e.search_ex(iq, prns, bins[-1:], 1)
    finally:
        e.close()
    assert tab[-1:].tobytes() == tab1.tobytes() and nbr[-1:].tobytes() == nbr1.tobytes()
    first = 512 - 13 * len(prns)                       # PRN index of cell 512 in the last bin
    assert prns[first:] == [32, 33, 34, 35, 36, 37]
    got = _records(tab[-1:, first:], nbr[-1:, first:])
    surf = {}
    ref = ar.acq_ref(iq, bins[-1:], prns[first:], cs, 1, surfaces=surf)
    ref, excused = _settle_argmax(got, ref, surf, 'second chunk')
    orc = ar.oracle_record_padded(iq, bins[-1:], prns[first:], cs, 1)
    _hold_to_oracle('second chunk of the 32768 pair', [got], [ref], [orc], excused)
