#!/usr/bin/env python3
"""Bit-synchronous tracking of refined hits (gpsmi_acq_track) beside the deep search and the
refinement of the same job, device time.

    python tools/acq_track_bench.py [--reps 25] [--json]
    python tools/acq_track_bench.py --stats kernel_stats.csv

Three points on the deep scene (tests/deep_ref.py), channels opened at the truth: CS 2048, 5 and 64
channels over 1 s (45 bits fit the 33 blocks: the time is scaled to 50 bits as well), CS 16368, 5
channels over 300 ms (12 bits).  Input is device resident; each time is gpsmi_acq_last_ms (HIP
events around the kernel), the median of --reps calls after a warm-up.  The 1-s deep search of
tools/acq_deep_bench.py and the 1000-ms refinement of tools/acq_refine_bench.py run in the same
job.  The kernel is one launch, so a kernel trace cannot split it: the split between the sample
loop and the one-thread update is the two-point fit  t / bit = update + samples / rate  through the
5-channel points at the two code lengths (40960 and 327360 samples per bit).  --stats summarises
the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests', 'tools'):
    sys.path.insert(0, os.path.join(ROOT, p))

POINTS = [dict(cs=2048, n_cyc=32, nch=5, n_bits=45), dict(cs=2048, n_cyc=32, nch=64, n_bits=45),
          dict(cs=16368, n_cyc=8, nch=5, n_bits=12)]


def run_point(pt, reps):
    from deep_ref import L1_HZ, deep_scene
    from gpsmi._lib import WTRK_STATE_DTYPE
    from gpsmi.engine import AcqEngine, Config, DeviceBuffer
    cs, nch, n_bits = pt['cs'], pt['nch'], pt['n_bits']
    sc = deep_scene(cs, pt['n_cyc'])
    n = (20 * n_bits + 3) * cs
    data = sc.block(0, n=n)
    buf = DeviceBuffer(data.nbytes)
    buf.upload(data)
    st = np.zeros(nch, WTRK_STATE_DTYPE)
    for i in range(nch):
        s = sc.sats[i % len(sc.sats)]
        st[i]['prn'], st[i]['f_hz'], st[i]['f_acc'] = s.prn, s.doppler, s.doppler
        st[i]['tau'] = s.delay / (1.0 + s.doppler / L1_HZ) + (cs if s.delay < 8 else 0)
    e = AcqEngine(Config(code_samples=cs, n_cyc=pt['n_cyc']))
    ms = []
    for r in range(reps + 3):
        _, out = e.track_weak((buf.ptr, n), st, n_bits)
        assert (out['bit_no'] == n_bits).all()
        if r >= 3:                                   # warm-up
            ms.append(e.last_ms())
    e.close()
    buf.free()
    med = float(np.median(ms))
    return dict(pt, track_ms=med, track_ms_min_max=[float(np.min(ms)), float(np.max(ms))],
                data_ms=20 * n_bits, us_per_bit=1e3 * med / n_bits, samples_per_bit=20 * cs, reps=reps)


def from_stats(path):
    import csv
    for r in csv.DictReader(open(path)):
        for k in ('wtrk_kernel', 'refine_prompt_kernel', 'refine_grid_kernel', 'refine_final_kernel',
                  'acq_spectrum_kernel<', 'acq_corr_kernel<2>'):
            if k in r['Name'].replace(' ', ''):
                print(f"{k:24s} calls {int(r['Calls']):4d}  mean {float(r['AverageNs']) / 1e3:9.1f} us"
                      f"  total {float(r['TotalDurationNs']) / 1e6:9.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--stats', help='summarise a kernel_stats.csv of this tool instead of running')
    a = ap.parse_args()
    if a.stats:
        from_stats(a.stats)
        return
    import acq_deep_bench
    import acq_refine_bench
    deep = acq_deep_bench.run_point(acq_deep_bench.POINTS[1], a.reps)
    ref = acq_refine_bench.run_point(acq_refine_bench.POINTS[0], a.reps)
    out = dict(deep_search_1s_ms=deep['deep_ms'], refine_1000ms_ms=ref['refine_ms'])
    print(json.dumps(out) if a.json else
          f"deep search 1 s: {deep['deep_ms']:.4f} ms; refinement of 5 hits over 1000 ms: {ref['refine_ms']:.4f} ms", flush=True)
    res = [run_point(pt, a.reps) for pt in POINTS]
    for r in res:
        print(json.dumps(r) if a.json else
              f"CS {r['cs']}: {r['nch']} channels x {r['n_bits']} bits ({r['data_ms']} ms of data): {r['track_ms']:.4f} ms"
              f" = {r['us_per_bit']:.2f} us per bit", flush=True)
    lo, hi = res[0], res[2]
    rate = (hi['samples_per_bit'] - lo['samples_per_bit']) / (hi['us_per_bit'] - lo['us_per_bit'])
    upd = lo['us_per_bit'] - lo['samples_per_bit'] / rate
    fit = dict(fit_update_us_per_bit=upd, fit_samples_per_us=rate,
               sample_loop_share_2048=1.0 - upd / lo['us_per_bit'], track_1s_50_bits_ms=lo['us_per_bit'] * 50 / 1e3)
    print(json.dumps(fit) if a.json else
          f"fit: update {upd:.2f} us per bit, sample loop {rate:.0f} samples per us per channel; at 2048 the sample "
          f"loop is {100 * fit['sample_loop_share_2048']:.0f} % of a bit; 50 bits: {fit['track_1s_50_bits_ms']:.3f} ms", flush=True)


if __name__ == '__main__':
    main()
