#!/usr/bin/env python3
"""Refinement of deep hits (gpsmi_acq_refine) beside the deep search that finds them, device time.

    python tools/acq_refine_bench.py [--reps 25] [--json]
    python tools/acq_refine_bench.py --stats kernel_stats.csv

Three points on the deep scene (tests/deep_ref.py), five hits each, +-120 Hz at 2 Hz: CS 2048 over
1000 ms and over 4000 ms, CS 16368 over 300 ms.  Input is device resident; each time is
gpsmi_acq_last_ms (HIP events around the three kernels), the median of --reps calls after a
warm-up.  The 1-s shape of tools/acq_deep_bench.py (31 SV x 51 bins, 250 x 4 ms) runs in the same
job and the ratio refine / deep search is reported for the 1000-ms point.  --stats summarises the
kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool: the prompt kernel's
bytes per second against what it reads tell whether the repeated reads of IQ come from the caches."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests', 'tools'):
    sys.path.insert(0, os.path.join(ROOT, p))

POINTS = [dict(cs=2048, n_cyc=32, n_ms=1000), dict(cs=2048, n_cyc=32, n_ms=4000),
          dict(cs=16368, n_cyc=8, n_ms=300)]


def run_point(pt, reps):
    from deep_ref import deep_scene
    from gpsmi.engine import AcqEngine, Config, DeviceBuffer
    from refine_ref import scene_cases
    cs, n_ms = pt['cs'], pt['n_ms']
    sc = deep_scene(cs, pt['n_cyc'])
    n = (n_ms + 2) * cs + 8
    one = min(n, 1002 * cs + 8)                      # (a second of scene, repeated: timing only)
    piece = sc.block(0, n=one)
    buf = DeviceBuffer(n * piece.itemsize)
    for k in range(0, n, one):
        m = min(one, n - k)
        buf.upload(piece[:m], k * piece.itemsize)
    hits = scene_cases(sc, n_ms, cs)['A'][1][:5]
    e = AcqEngine(Config(code_samples=cs, n_cyc=pt['n_cyc']))
    ms = []
    for r in range(reps + 3):
        e.refine((buf.ptr, n), hits, n_ms)
        if r >= 3:                                   # warm-up
            ms.append(e.last_ms())
    e.close()
    buf.free()
    med = float(np.median(ms))
    return dict(pt, nhits=len(hits), n_df=121, refine_ms=med, refine_ms_min_max=[float(np.min(ms)), float(np.max(ms))],
                iq_bytes_read=int(len(hits) * n_ms * (cs + 2 * (1 if cs == 2048 else 8)) * 8),
                reps=reps)


STAT_KERNELS = ['refine_prompt_kernel', 'refine_grid_kernel', 'refine_final_kernel',
                'acq_spectrum_kernel<', 'acq_corr_kernel<2>']


def from_stats(path):
    import csv
    for r in csv.DictReader(open(path)):
        for k in STAT_KERNELS:
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
    deep = acq_deep_bench.run_point(acq_deep_bench.POINTS[1], a.reps)
    out = dict(deep_search_1s_ms=deep['deep_ms'], deep_search_1s_ms_min_max=deep['deep_ms_min_max'])
    print(json.dumps(out) if a.json else f"deep search, 31 SV x 51 bins x 250 x 4 ms: {deep['deep_ms']:.4f} ms",
          flush=True)
    for pt in POINTS:
        r = run_point(pt, a.reps)
        if pt is POINTS[0]:
            r['refine_over_deep_search'] = r['refine_ms'] / deep['deep_ms']
        if a.json:
            print(json.dumps(r), flush=True)
        else:
            print(f"CS {r['cs']}: {r['nhits']} hits x {r['n_ms']} ms x {r['n_df']} df: refine {r['refine_ms']:.4f} ms"
                  + (f", refine / deep search {r['refine_over_deep_search']:.3f}" if pt is POINTS[0] else ''),
                  flush=True)


if __name__ == '__main__':
    main()
