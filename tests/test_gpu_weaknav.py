"""GPU: weak channels into datagrams and the position fix (gpsmi.weaknav, pipeline.WeakAssist,
DESIGN.md 4.2h) on the scenes of weaknav_scene.py.

Clock: the receiver stamps the first sample of block n (from 0) with (n + 1) ngps, so a true arrival
at stream sample k reads k + ngps there; every truth below is moved onto that clock.

Bounds.  The tracker's asserted tau tolerance is 0.25 sample; in metres at a PDOP
of 3 that caps a single fix at 0.25 c / fs * 3 = 109.8 m and the mean of the later half at 36.6 m.
Measured on the first MI355X run: see FIX_WORST_M / FIX_MEAN_M; asserted at twice
each, under the caps.
A frame's ST is a whole number, int(rint(tau)), so ST itself can sit up to 0.5 sample from any
truth; what is held to 0.25 sample is the unrounded tau of the frame's first bit
(WeakChannelNav.frame_tau), and ST must be exactly its rounding.
Frames of the two paths are compared in the fields evalGpsBits decodes and 'SAT'; 'AMP', 'CRM' and
'FRQ' are each path's own display measurements."""
import pickle

import numpy as np
import pytest

from gpsmi import navbits as nb, position as P, synth_nav, weaknav as WN
import weaknav_scene as S
from weaknav_truth import arrival

pytestmark = pytest.mark.gpu

CS, NGPS = 2048, 65536
C_LIGHT = 299792458.0
CAP_SINGLE_M = 0.25 * C_LIGHT / (1000.0 * CS) * 3.0
CAP_MEAN_M = 0.25 * C_LIGHT / (1000.0 * CS)
FIX_WORST_M, FIX_MEAN_M = 27.31, 10.57          # MI355X, first run: 62 fixes, median 14.71 m
DECODED = {k for keys in nb.FRAME_KEYS.values() for k in keys} - {'ST'} | {'SAT'}


def true_starts(sat):
    """Arrival of every code start of the scene on the receiver's clock."""
    return arrival(sat, np.arange(-4000, 12000), CS) + NGPS


def co_ph_errors(sat, entries):
    starts = true_starts(sat)
    c = np.array([s for s, _ in entries]) * NGPS + NGPS // 2
    t = starts[np.searchsorted(starts, c, side='right') - 1]
    return (np.array([cp for _, cp in entries]) - t % CS + CS / 2) % CS - CS / 2


def run_receiver(make, blocks):
    """-> (the object, [(block, datagram bytes)], act_sat_set seen over the run)."""
    rx = make()
    out, seen = [], set()
    for b, blk in enumerate(blocks):
        dg = rx.feed(blk)
        seen |= set(getattr(rx, 'rx', rx).act_sat_set)
        if dg is not None:
            out.append((b, dg))
    rx.drain()
    return rx, out, seen


def solve(datagrams, ephs):
    solver = P.PositionSolver(ephemerides=ephs)
    fixes = []
    for dg in datagrams:
        fixes += solver.feed(pickle.loads(dg))
    return fixes


@pytest.fixture(scope='module')
def mixed_run():
    """The mixed scene through a plain Receiver and through WeakAssist, once."""
    from gpsmi.pipeline import Receiver, WeakAssist
    sc, info, low = S.mixed()
    blocks = S.mixed_blocks()
    rx, plain, seen = run_receiver(Receiver, blocks)
    rx.close()
    wa, _, _ = run_receiver(lambda: WeakAssist(Receiver()), blocks)
    keep = dict(plain=plain, seen=seen, result_list=list(wa.result_list), refined=wa.refined.copy(),
                kept_start=wa._kept_start, chan=dict(wa.handoff.chan), weak_prns=wa.weak_prns)
    wa.close()
    return keep


# ---- 1. mixed scene to fix ------------------------------------------------------------------------

def test_mixed_scene_to_fix(mixed_run):
    sc, info, low = S.mixed()
    r = mixed_run
    # the plain receiver: three satellites, no fix
    assert not r['seen'] & set(low) and len(r['seen']) == 3
    assert solve([dg for _, dg in r['plain']], info['ephs']) == []
    # the assisted one: the three lowered satellites acquired, tracked and decoded
    assert sorted(r['weak_prns']) == low
    for prn in low:
        sat = next(s for s in sc.sats if s.prn == prn)
        frames = r['chan'][prn].frames
        assert len(frames) >= 1
        for f in frames:
            n = f['tow'] - info['tow0']
            status, want = nb.extract_subframe(np.asarray(sat.nav_bits)[300 * n:300 * n + 300])
            assert status == nb.NO_ERR and {k: v for k, v in f.items() if k != 'ST'} == want
            assert f['ID'] == n % 5 + 1
    fixes = solve(r['result_list'], info['ephs'])
    assert len(fixes) > 30
    xyz = np.array([f[1:] for f in fixes])
    err = np.linalg.norm(xyz - S.TRUTH, axis=1)
    late = xyz[len(xyz) // 2:]
    mean_err = float(np.linalg.norm(late.mean(axis=0) - S.TRUTH))
    print('mixed scene: %d fixes, worst single-fix error %.2f m, median %.2f m, mean of the later half off by %.2f m'
          % (len(fixes), err.max(), np.median(err), mean_err))
    assert err.max() <= min(2.0 * FIX_WORST_M, CAP_SINGLE_M)
    assert mean_err <= min(2.0 * FIX_MEAN_M, CAP_MEAN_M)


# ---- 2. one satellite, both paths -----------------------------------------------------------------

def test_one_satellite_both_paths():
    from gpsmi.acquisition import open_weak_channels
    from gpsmi.pipeline import Receiver, WeakTracker, largest_peak_hits, refine_centred
    sc, info = S.one()
    blocks = S.one_blocks()
    sat = min(sc.sats, key=lambda s: abs(s.doppler))
    prn = sat.prn
    rx, dgs, _ = run_receiver(Receiver, blocks)
    try:
        assert prn in rx.act_sat_set
        cfg, acq = rx.cfg, rx.acq
        first = 25                                    # the block behind the cold sweep
        whole = np.concatenate(blocks[first:first + 33])
        freqs = [cfg.min_freq + cfg.step_freq * i for i in range(int(round((cfg.max_freq - cfg.min_freq) / cfg.step_freq)))]
        found = largest_peak_hits(acq, whole[:1000 * CS], [prn], freqs)
        _, rec, _ = refine_centred(acq, whole, found)
        assert len(rec) == 1 and rec[0]['confirmed'] == 1 and rec[0]['code_phase'] >= 0
        clock = (first + 1) * NGPS
        trk = WeakTracker(acq.engine, open_weak_channels(rec, cfg, data_start=clock), clock)
        ch = WN.WeakChannelNav(prn, cfg)
        for i in range(first, len(blocks), 16):
            ch.absorb(trk.push(np.concatenate(blocks[i:i + 16]))[0])
    finally:
        rx.close()
    strong = [pickle.loads(dg) for _, dg in dgs]
    s_frames = [f for dg in strong for f in dg[1] if f.get('SAT') == prn and 'ID' in f]
    s_co_ph = dict(e for dg in strong for e in dg[2].get(prn, []))
    assert len(s_frames) >= 1 and len(ch.frames) == len(s_frames)
    starts = true_starts(sat)
    for fw, tau, fs in zip(ch.frames, ch.frame_tau, s_frames):
        assert {k: v for k, v in fw.items() if k != 'ST'} == {k: v for k, v in fs.items() if k in DECODED and k != 'SAT'}
        t = starts[4000 + 20 * 300 * (fw['tow'] - info['tow0'])]
        print('PRN %d subframe tow %d: true arrival %.3f, weak tau %+.3f ST %+.3f, receiver ST %+.3f (samples off)'
              % (prn, fw['tow'], t, tau - t, fw['ST'] - t, fs['ST'] - t))
        assert abs(tau - t) <= 0.25 and fw['ST'] == int(np.rint(tau))
        assert fw['ST'] // CS == fs['ST'] // CS
    common = sorted(set(s_co_ph) & dict(ch.co_ph).keys())
    assert len(common) > 150
    w = co_ph_errors(sat, [(s, dict(ch.co_ph)[s]) for s in common])
    r = co_ph_errors(sat, [(s, s_co_ph[s]) for s in common])
    print('PRN %d coPh against the truth on %d common blocks: weak rms %.4f worst %.4f (block %d), receiver rms %.4f worst %.4f sample'
          % (prn, len(common), np.sqrt((w ** 2).mean()), np.abs(w).max(), common[int(np.abs(w).argmax())],
             np.sqrt((r ** 2).mean()), np.abs(r).max()))
    assert np.abs(w).max() < 0.25


# ---- 3. chunking ----------------------------------------------------------------------------------

def test_one_call_and_chunks_of_16_blocks_give_the_same_datagrams(mixed_run):
    from gpsmi.acquisition import Acquisition, open_weak_channels
    from gpsmi.engine import Config
    from gpsmi.pipeline import WeakTracker
    r = mixed_run
    cfg = Config()
    rec = r['refined'][(r['refined']['confirmed'] == 1) & (r['refined']['code_phase'] >= 0)]
    start = r['kept_start']
    first = start // NGPS - 1
    blocks = S.mixed_blocks()
    acq = Acquisition(cfg)
    out = []
    try:
        for step in (len(blocks), 16):
            states = open_weak_channels(rec, cfg, data_start=start)
            trk = WeakTracker(acq.engine, states, start)
            ho = WN.WeakHandoff(cfg)
            for p in states['prn']:
                ho.open(p)
            dgs = []
            for i in range(first, len(blocks), step):
                for p, new in zip(states['prn'], trk.push(np.concatenate(blocks[i:i + step]))):
                    ho.absorb(p, new)
                dgs += ho.datagrams()
            out.append(dgs)
    finally:
        acq.engine.close()
    assert len(out[0]) >= 7 and [s for s, _ in out[0]] == [s for s, _ in out[1]]
    assert pickle.dumps(out[0]) == pickle.dumps(out[1])
    for (_, a), (_, b) in zip(out[0], out[1]):
        assert pickle.dumps(a) == pickle.dumps(b)
    # ... and they are what WeakAssist merged in
    merged = {WN.report_stream(t): t for t in map(pickle.loads, r['result_list'])}
    n_same = 0
    for s, (_, frames, co_ph) in out[1]:
        for p, lst in co_ph.items():
            if s in merged and p in merged[s][2]:
                assert merged[s][2][p] == lst
                n_same += 1
    assert n_same >= 15


# ---- 4. pass-through ------------------------------------------------------------------------------

def test_all_strong_scene_passes_through():
    from gpsmi.pipeline import Receiver, WeakAssist
    sc, info = synth_nav.geometric_scene(S.TRUTH, 22.0)           # test_iq_to_position_fix's scene
    blocks = [sc.block(b) for b in range(125)]                    # its first 4 s
    rx, plain, _ = run_receiver(Receiver, blocks)
    rx.close()
    wa, got, _ = run_receiver(lambda: WeakAssist(Receiver()), blocks)
    searched, weak = wa.searched, wa.weak_prns
    wa.close()
    assert searched and weak == []
    assert len(plain) >= 3 and got == plain
