#!/usr/bin/env python3
"""Non-coherent search against the coherent one on the same grid (gpsmi_acq_search_nc vs
gpsmi_acq_search), device time per cell.

    python tools/acq_nc_bench.py [--reps 25] [--cpu] [--json]

Two points: CS 2048, 31 SV x 51 bins, n_coh 4, n_seg 25 (100 ms); CS 16368, 12 SV x 21 bins,
n_coh 8, n_seg 25 (200 ms).  After a warm-up the two calls alternate in one run; each time is
gpsmi_acq_last_ms (HIP events around the kernels, uploads excluded: device-resident input), and
the median of --reps calls is reported.  Per cell: coherent ms / (SV x bin), non-coherent
ms / (segment x SV x bin).  FLOP/s: 5 N log2 N per transform -- at 2048 one forward per
(segment, bin) and one inverse per (segment, SV, bin); at 16368 the forward and the inverse of
every (segment, SV, bin) (the native kernel transforms the folded samples per cell).  --cpu
also times the numpy restatement (tests/test_acq_noncoherent.py:nc_table, one core) of the 2048
search."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

POINTS = [dict(cs=2048, n_cyc=32, nsv=31, nbins=51, n_coh=4, n_seg=25),
          dict(cs=16368, n_cyc=8, nsv=12, nbins=21, n_coh=8, n_seg=25)]


def flops(pt):
    n = pt['cs']
    per = 5.0 * n * math.log2(n)
    cells = pt['n_seg'] * pt['nsv'] * pt['nbins']
    if n == 2048:
        return per * (pt['n_seg'] * pt['nbins'] + cells)
    return per * 2 * cells


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
    coh, nc = [], []
    for r in range(reps + 3):
        e.search((buf.ptr, n), prns, freqs, pt['n_coh'])
        c = e.last_ms()
        e.search_noncoherent((buf.ptr, n), prns, freqs, pt['n_coh'], pt['n_seg'])
        m = e.last_ms()
        if r >= 3:                                  # warm-up
            coh.append(c)
            nc.append(m)
    e.close()
    buf.free()
    cmed, nmed = float(np.median(coh)), float(np.median(nc))
    cells = pt['nsv'] * pt['nbins']
    out = dict(pt, coherent_ms=cmed, noncoherent_ms=nmed,
               coherent_ns_per_cell=cmed * 1e6 / cells,
               noncoherent_ns_per_cell=nmed * 1e6 / (cells * pt['n_seg']),
               noncoherent_tflops=flops(pt) / (nmed * 1e-3) / 1e12, reps=reps)
    out['bar_met'] = out['noncoherent_ns_per_cell'] <= out['coherent_ns_per_cell']
    return out


def cpu_time(pt):
    import gps_oracle as orc
    from gpsmi import synth
    from test_acq_noncoherent import nc_table
    cs = pt['cs']
    sc = synth.default_scene(12, seed=7, code_samples=cs, n_cyc=pt['n_cyc'])
    data = sc.block(0, n=pt['n_seg'] * pt['n_coh'] * cs)
    prns = list(range(2, 2 + pt['nsv']))
    freqs = [-200.0 * (pt['nbins'] // 2) + 200.0 * i for i in range(pt['nbins'])]
    t0 = time.perf_counter()
    nc_table(data, freqs, prns, pt['n_coh'], pt['n_seg'], orc.Params(code_samples=cs, n_cyc=pt['n_cyc']))
    return (time.perf_counter() - t0) * 1e3


# kernels of the non-coherent search -> (point, transforms per call they carry).  The wipe-off folds
# also serve the coherent search this tool alternates with (one segment a launch): their rows of a
# trace hold both searches' launches, the FLOP/s of that row is an upper bound
STAT_KERNELS = {'acq_spectrum_kernel<': (0, lambda p: p['n_seg'] * p['nbins']),
                'acq_corr_kernel<1>': (0, lambda p: p['n_seg'] * p['nsv'] * p['nbins']),
                'acq_fold_kernel<': (1, lambda p: 0),
                'pfa_corr_kernel<2>': (1, lambda p: 2 * p['n_seg'] * p['nsv'] * p['nbins'])}


def from_stats(path):
    """Kernel times of a rocprofv3 --kernel-trace --stats run of this tool (kernel_stats.csv) and
    the FLOP/s of the transforms each kernel carries (5 N log2 N per transform)."""
    import csv
    for r in csv.DictReader(open(path)):
        for k, (pi, ntr) in STAT_KERNELS.items():
            if k in r['Name'].replace(' ', ''):
                pt = POINTS[pi]
                avg = float(r['AverageNs'])
                f = 5.0 * pt['cs'] * math.log2(pt['cs']) * ntr(pt)
                print(f"{k:24s} calls {int(r['Calls']):4d}  mean {avg / 1e3:8.1f} us"
                      + (f"  {f / avg / 1e3:6.1f} TFLOP/s" if f else ''))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--stats', help='summarise a kernel_stats.csv of this tool instead of running')
    a = ap.parse_args()
    if a.stats:
        from_stats(a.stats)
        return
    res = [run_point(pt, a.reps) for pt in POINTS]
    if a.cpu:
        res[0]['cpu_restatement_ms'] = cpu_time(POINTS[0])
    for r in res:
        if a.json:
            print(json.dumps(r))
        else:
            print(f"CS {r['cs']}: {r['nsv']} SV x {r['nbins']} bins, n_coh {r['n_coh']}: coherent "
                  f"{r['coherent_ms']:.4f} ms ({r['coherent_ns_per_cell']:.2f} ns/cell); "
                  f"x {r['n_seg']} segments {r['noncoherent_ms']:.4f} ms "
                  f"({r['noncoherent_ns_per_cell']:.2f} ns/cell, {r['noncoherent_tflops']:.2f} "
                  f"TFLOP/s by 5 N log2 N); bar {'met' if r['bar_met'] else 'MISSED'}"
                  + (f"; numpy restatement {r['cpu_restatement_ms']:.0f} ms"
                     if 'cpu_restatement_ms' in r else ''))


if __name__ == '__main__':
    main()
