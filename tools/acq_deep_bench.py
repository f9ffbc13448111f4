#!/usr/bin/env python3
"""Deep search against the non-coherent one on the same grid (gpsmi_acq_search_deep vs
gpsmi_acq_search_nc), device time per (segment x SV x bin) cell.

    python tools/acq_deep_bench.py [--reps 25] [--json]
    python tools/acq_deep_bench.py --stats kernel_stats.csv

Three points, DESIGN.md 4.2a's shapes: CS 2048, 31 SV x 51 bins, n_coh 4, n_seg 25 (100 ms) and
n_seg 250 (1 s); CS 16368, 12 SV x 21 bins, n_coh 8, n_seg 25 (200 ms).  After a warm-up the two
calls alternate in one run on device-resident input; each time is gpsmi_acq_last_ms (HIP events
around the kernels), and the median of --reps calls is reported, with the ratio deep / non-coherent.
The deep search adds one LDS round trip of the magnitudes per segment and, at 16368, two workgroup
barriers.  --stats summarises the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of
this tool (counters, if wanted, in a run of their own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

POINTS = [dict(cs=2048, n_cyc=32, nsv=31, nbins=51, n_coh=4, n_seg=25),
          dict(cs=2048, n_cyc=32, nsv=31, nbins=51, n_coh=4, n_seg=250),
          dict(cs=16368, n_cyc=8, nsv=12, nbins=21, n_coh=8, n_seg=25)]


def run_point(pt, reps):
    from gpsmi import synth
    from gpsmi.engine import AcqEngine, Config, DeviceBuffer
    cs = pt['cs']
    sc = synth.default_scene(12, seed=7, code_samples=cs, n_cyc=pt['n_cyc'])
    n = pt['n_seg'] * pt['n_coh'] * cs
    data = sc.block(0, n=n)
    buf = DeviceBuffer(data.nbytes)
    buf.upload(data)
    prns = list(range(2, 2 + pt['nsv']))
    freqs = [-200.0 * (pt['nbins'] // 2) + 200.0 * i for i in range(pt['nbins'])]
    e = AcqEngine(Config(code_samples=cs, n_cyc=pt['n_cyc']))
    nc, deep = [], []
    for r in range(reps + 3):
        e.search_noncoherent((buf.ptr, n), prns, freqs, pt['n_coh'], pt['n_seg'])
        a = e.last_ms()
        e.search_deep((buf.ptr, n), prns, freqs, pt['n_coh'], pt['n_seg'])
        b = e.last_ms()
        if r >= 3:                                  # warm-up
            nc.append(a)
            deep.append(b)
    e.close()
    buf.free()
    nmed, dmed = float(np.median(nc)), float(np.median(deep))
    cells = pt['nsv'] * pt['nbins'] * pt['n_seg']
    return dict(pt, noncoherent_ms=nmed, deep_ms=dmed,
                noncoherent_ns_per_cell=nmed * 1e6 / cells, deep_ns_per_cell=dmed * 1e6 / cells,
                deep_over_noncoherent=dmed / nmed,
                noncoherent_ms_min_max=[float(np.min(nc)), float(np.max(nc))],
                deep_ms_min_max=[float(np.min(deep)), float(np.max(deep))], reps=reps)


STAT_KERNELS = ['acq_spectrum_kernel<', 'acq_corr_kernel<1>', 'acq_corr_kernel<2>',
                'acq_fold_kernel<', 'pfa_corr_kernel<2>', 'pfa_corr_kernel<3>']


def from_stats(path):
    """Kernel times of a rocprofv3 --kernel-trace --stats run of this tool (kernel_stats.csv): calls,
    mean and total per kernel of the two searches (the three points share the kernels: the mean
    mixes them, the totals compare the two searches over the same work)."""
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
    for pt in POINTS:
        r = run_point(pt, a.reps)
        if a.json:
            print(json.dumps(r), flush=True)
        else:
            print(f"CS {r['cs']}: {r['nsv']} SV x {r['nbins']} bins, n_coh {r['n_coh']} x {r['n_seg']} "
                  f"segments: non-coherent {r['noncoherent_ms']:.4f} ms ({r['noncoherent_ns_per_cell']:.2f} "
                  f"ns/cell), deep {r['deep_ms']:.4f} ms ({r['deep_ns_per_cell']:.2f} ns/cell), "
                  f"deep / non-coherent {r['deep_over_noncoherent']:.3f}", flush=True)


if __name__ == '__main__':
    main()
