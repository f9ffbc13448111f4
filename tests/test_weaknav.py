"""CPU: gpsmi.weaknav -- bit records of the bit-synchronous tracker to subframes, code phases
and hand-off datagrams -- on records built from a geometric scene's truth, no IQ.

The scene is geometric_scene(truth, 14 s, n_sats=5); the records start at bit 37 (mid-subframe, not
word-aligned).  14 s hold ONE subframe wholly behind bit 37 (bits 300..599), so the polarity-flip
case, which needs three, reads the same kind of records off a 26-s scene (bits 300..1199); nothing
else differs.  Tolerances: ST is a rounded position, 0.5 sample; coPh 2e-3 sample -- the scene's
polynomial is good to 1e-3 (fit_err_samples, asserted) and a record's Tc from the Doppler at the
bit's start drifts by less than that over 20 ms at under 2 Hz/s (20 ms * 2 Hz/s / L1 * 20 periods
* cs < 1e-6 sample)."""
import functools
import pickle

import numpy as np
import pytest

from gpsmi import navbits as nb, position as P, synth_nav, weaknav as WN
from gpsmi.engine import Config
from weaknav_truth import arrival, truth_records

SECONDS, B0 = 14.0, 37
TRUTH = np.array(P.geo_to_ecef(49.082961, 8.307581, 160.0))


@functools.lru_cache(maxsize=None)
def scene(cs=2048, n_cyc=32, seconds=SECONDS):
    sc, info = synth_nav.geometric_scene(TRUTH, seconds, n_sats=5, code_samples=cs, n_cyc=n_cyc)
    assert info['fit_err_samples'] < 1e-3
    recs = {s.prn: truth_records(s, cs, B0, seconds * 1000 * cs) for s in sc.sats}
    return sc, info, recs


def absorbed(prn, rec, cfg, chunk):
    ch = WN.WeakChannelNav(prn, cfg)
    for i in range(0, len(rec), chunk):
        ch.absorb(rec[i:i + chunk])
    return ch


def expected_frames(sat, bits, cs):
    """Every subframe wholly behind the first bit and ending a bit before the last: (fields of
    extract_subframe of the transmitted bits, true arrival of the first bit)."""
    out = []
    for start in range(-(-int(bits[0]) // 300) * 300, int(bits[-1]) - 300 + 1, 300):
        status, f = nb.extract_subframe(np.asarray(sat.nav_bits)[start:start + 300])
        assert status == nb.NO_ERR
        out.append((f, float(arrival(sat, 20 * start, cs))))
    return out


def check_frames(frames, want):
    assert len(frames) == len(want)
    for got, (f, t) in zip(frames, want):
        assert {k: v for k, v in got.items() if k != 'ST'} == f
        assert list(got) == nb.FRAME_KEYS[f['ID']]
        assert isinstance(got['ST'], int) and abs(got['ST'] - t) <= 0.5, (got['ST'], t)


# ---- 1. frames ------------------------------------------------------------------------------------

def test_frames_in_any_chunking_and_polarity():
    sc, info, recs = scene()
    cfg = Config()
    for s in sc.sats:
        rec, bits = recs[s.prn]
        want = expected_frames(s, bits, 2048)
        assert len(want) == 1 and want[0][0]['tow'] == info['tow0'] + 1 and want[0][0]['ID'] == 2
        ref = absorbed(s.prn, rec, cfg, 300).frames
        check_frames(ref, want)
        for chunk in (1, 7, 25):
            assert absorbed(s.prn, rec, cfg, chunk).frames == ref
        neg = rec.copy()
        neg['p_i'] = -neg['p_i']
        assert absorbed(s.prn, neg, cfg, 25).frames == ref


def test_polarity_flip_costs_one_subframe():
    """26 s: subframes at bits 300, 600 and 900 lie behind bit 37.  With every bit negated from the
    middle of word 5 of the second on, the second fails its parity, the first and the third are
    returned, the third as without the flip."""
    sc, info = synth_nav.geometric_scene(TRUTH, 26.0, n_sats=2)
    cfg = Config()
    for s in sc.sats:
        rec, bits = truth_records(s, 2048, B0, 26.0 * 1000 * 2048)
        want = expected_frames(s, bits, 2048)
        assert [f['ID'] for f, _ in want] == [2, 3, 4]
        clean = absorbed(s.prn, rec, cfg, 25).frames
        check_frames(clean, want)
        flip = rec.copy()
        at = 600 + 4 * 30 + 15 - B0
        flip['p_i'][at:] = -flip['p_i'][at:]
        for chunk in (1, 25, 300):
            got = absorbed(s.prn, flip, cfg, chunk).frames
            assert got == [clean[0], clean[2]]


# ---- 2. code phases -------------------------------------------------------------------------------

@pytest.mark.parametrize('cs,n_cyc', [(2048, 32), (16368, 8)])
def test_code_phases_at_the_block_centres(cs, n_cyc):
    seconds = SECONDS if cs == 2048 else 3.0
    sc, info, recs = scene(cs, n_cyc, seconds)
    cfg = Config(code_samples=cs, n_cyc=n_cyc)
    ngps = cfg.ngps
    for s in sc.sats:
        rec, bits = recs[s.prn]
        ch = absorbed(s.prn, rec, cfg, 25)
        starts = arrival(s, np.arange(20 * bits[0], 20 * (bits[-1] + 1) + 1), cs)
        first, end = starts[0], starts[-1]
        blocks = [b for b, _ in ch.co_ph]
        lo, hi = int(np.ceil(first / ngps)), int(end // ngps)
        assert blocks == list(range(lo, hi)) and len(blocks) > 50
        worst = 0.0
        for b, cp in ch.co_ph:
            assert isinstance(b, int) and isinstance(cp, float) and 0 <= cp < cs
            c = b * ngps + ngps // 2
            t = starts[np.searchsorted(starts, c, side='right') - 1]      # the period covering c
            d = (cp - t % cs + cs / 2) % cs - cs / 2
            worst = max(worst, abs(d))
        print('cs %d PRN %d: %d blocks, worst coPh error %.2e sample' % (cs, s.prn, len(blocks), worst))
        assert worst <= 2e-3


def test_zero_tail_behind_data_end_reports_nothing():
    sc, info, recs = scene()
    cfg = Config()
    s = sc.sats[0]
    rec, _ = recs[s.prn]
    whole = absorbed(s.prn, rec[:120], cfg, 40)
    tail = np.concatenate([rec[:120], np.zeros(30, rec.dtype)])
    ch = WN.WeakChannelNav(s.prn, cfg)
    ch.absorb(tail[:70])
    ch.absorb(tail[70:])
    ch.absorb(tail[:0])
    assert ch.n_bits == 120 and ch.co_ph == whole.co_ph and ch.covered_end == whole.covered_end
    assert ch.co_ph[-1][0] == int(whole.covered_end // cfg.ngps) - 1


# ---- 3. solver ------------------------------------------------------------------------------------

def handoff_datagrams(prns, recs, cfg, chunk=25):
    ho = WN.WeakHandoff(cfg)
    for p in prns:
        ho.open(p)
    out = []
    n = max(len(recs[p][0]) for p in prns)
    for i in range(0, n, chunk):
        for p in prns:
            ho.absorb(p, recs[p][0][i:i + chunk])
        out += ho.datagrams()
    return out


def check_fixes(fixes):
    assert len(fixes) > 20
    xyz = np.array([f[1:] for f in fixes])
    late = xyz[len(xyz) // 2:]
    err = np.linalg.norm(late.mean(axis=0) - TRUTH)
    print('%d fixes, mean of the later half off truth by %.3f m' % (len(fixes), err))
    assert err < 5.0


def test_weak_only_datagrams_give_the_fix():
    sc, info, recs = scene()
    cfg = Config()
    prns = [s.prn for s in sc.sats]
    dgs = handoff_datagrams(prns, recs, cfg)
    assert [s for s, _ in dgs] == list(range(dgs[0][0], dgs[-1][0] + 1, 32)) and dgs[0][0] % 32 == 0
    assert dgs == handoff_datagrams(prns, recs, cfg, chunk=1000)
    solver = P.PositionSolver(ephemerides=info['ephs'])
    fixes = []
    for _, dg in dgs:
        assert dg[0] == 0 and {f['SAT'] for f in dg[1]} == set(prns)
        fixes += solver.feed(pickle.loads(pickle.dumps(dg)))
    check_fixes(fixes)


def test_three_strong_two_merged_give_the_fix():
    sc, info, recs = scene()
    cfg = Config()
    prns = [s.prn for s in sc.sats]
    strong = dict(handoff_datagrams(prns[:3], recs, cfg))
    weak = dict(handoff_datagrams(prns[3:], recs, cfg))
    alone, merged = P.PositionSolver(ephemerides=info['ephs']), P.PositionSolver(ephemerides=info['ephs'])
    fixes = []
    for s in sorted(set(strong) | set(weak)):
        if s in strong:
            assert alone.feed(strong[s]) == []                  # three satellites: no fix
        fixes += merged.feed(WN.merge_datagrams(strong.get(s), weak.get(s)))
    check_fixes(fixes)


# ---- 4. merge -------------------------------------------------------------------------------------

def test_merge():
    sc, info, recs = scene()
    cfg = Config()
    prns = [s.prn for s in sc.sats]
    strong = handoff_datagrams(prns[:3], recs, cfg)[-1][1]
    weak = handoff_datagrams(prns[2:], recs, cfg)[-1][1]        # prns[2] on both sides
    strong = (4711,) + strong[1:]
    m = WN.merge_datagrams(strong, weak)
    assert m[0] == 4711
    assert len(m[1]) == 5 and all(a is b for a, b in zip(m[1], strong[1]))
    assert [f['SAT'] for f in m[1]] == prns
    assert list(m[2]) == prns and all(m[2][p] is strong[2][p] for p in prns[:3])
    assert all(m[2][p] is weak[2][p] for p in prns[3:])
    assert len(strong[1]) == 3 and list(strong[2]) == prns[:3]  # the inputs are left as they were
    assert WN.merge_datagrams(strong, None) is strong and WN.merge_datagrams(None, weak) is weak
    assert WN.merge_datagrams(None, None) is None
    b = pickle.dumps(strong)
    assert pickle.dumps(WN.merge_datagrams(pickle.loads(b), None)) == b
    assert WN.report_stream(strong) == strong[2][prns[0]][-1][0]


# ---- 5. gap ---------------------------------------------------------------------------------------

def test_a_bit_no_gap_discards_the_pending_bits():
    """The records of bits 37..349 and, after a re-opening, of 350..686 with bit_no starting over:
    the subframe at 300..599 spans the gap and must not be returned, although every bit of it was
    absorbed; without the gap in bit_no it is."""
    sc, info, recs = scene()
    cfg = Config()
    s = sc.sats[1]
    rec, bits = recs[s.prn]
    cut = 350 - B0
    again = rec[cut:].copy()
    again['bit_no'] -= again['bit_no'][0]
    ch = WN.WeakChannelNav(s.prn, cfg)
    ch.absorb(rec[:cut])
    ch.absorb(again)
    assert ch.frames == [] and ch.n_bits == len(again)
    assert [b for b, _ in ch.co_ph] == sorted({b for b, _ in ch.co_ph})
    assert len(absorbed(s.prn, rec, cfg, cut).frames) == 1
    with pytest.raises(ValueError):
        WN.WeakChannelNav(s.prn, cfg).absorb(rec[::2])
