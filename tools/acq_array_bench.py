#!/usr/bin/env python3
"""Array search against A deep searches of the same rows (gpsmi_acq_search_array vs A calls of
gpsmi_acq_search_deep: the kernel there was before and the honest alternative), device time.

    python tools/acq_array_bench.py [--reps 15] [--antennas 2 3 4] [--json]
    python tools/acq_array_bench.py --stats kernel_stats.csv

One shape, DESIGN.md 4.2s's: CS 2048, 31 SV x 51 bins, 250 segments of 4 ms (one second), for A = 2, 3
and 4.  After a warm-up the array call and the A deep calls alternate in one run on device-resident
rows; each time is gpsmi_acq_last_ms (HIP events around the call's kernels, the spectra included),
the deep time the sum over the A rows, and the median of --reps rounds is reported with the ratio
array / deep.  Both do A transforms per segment and cell; the array kernel keeps 1 + A (A - 1)
accumulators per lag where the deep one keeps one, and runs at two waves per SIMD where that runs at
four.  --stats summarises the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this
tool (counters, if wanted, in a run of their own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

POINT = dict(cs=2048, n_cyc=32, nsv=31, nbins=51, n_coh=4, n_seg=250)


def run_point(pt, A, reps):
    from gpsmi import synth
    from gpsmi.engine import AcqEngine, Config, DeviceBuffer
    cs = pt['cs']
    sc = synth.default_scene(12, seed=7, code_samples=cs, n_cyc=pt['n_cyc'])
    n = pt['n_seg'] * pt['n_coh'] * cs
    row = sc.block(0, n=n)
    data = np.ascontiguousarray(np.stack([np.roll(row, 1000 * a) for a in range(A)]))   # (the times do not depend on it)
    buf = DeviceBuffer(data.nbytes)
    buf.upload(data)
    prns = list(range(2, 2 + pt['nsv']))
    freqs = [-200.0 * (pt['nbins'] // 2) + 200.0 * i for i in range(pt['nbins'])]
    e = AcqEngine(Config(code_samples=cs, n_cyc=pt['n_cyc']))
    arr, deep = [], []
    for r in range(reps + 2):
        e.search_array((buf.ptr, n), A, prns, freqs, pt['n_coh'], pt['n_seg'])
        a = e.last_ms()
        b = 0.0
        for k in range(A):
            e.search_deep((buf.at(k * n * 8), n), prns, freqs, pt['n_coh'], pt['n_seg'])
            b += e.last_ms()
        if r >= 2:                                  # warm-up
            arr.append(a)
            deep.append(b)
    e.close()
    buf.free()
    amed, dmed = float(np.median(arr)), float(np.median(deep))
    return dict(pt, antennas=A, array_ms=amed, deep_calls_ms=dmed, array_over_deep=amed / dmed,
                array_ms_min_max=[float(np.min(arr)), float(np.max(arr))],
                deep_calls_ms_min_max=[float(np.min(deep)), float(np.max(deep))], reps=reps)


STAT_KERNELS = ['acq_spectrum_kernel<', 'acq_corr_kernel<2>', 'acq_corr_array_kernel<2>', 'acq_corr_array_kernel<3>',
                'acq_corr_array_kernel<4>']


def from_stats(path):
    """Kernel times of a rocprofv3 --kernel-trace --stats run of this tool (kernel_stats.csv): calls,
    mean and total per kernel."""
    import csv
    for r in csv.DictReader(open(path)):
        for k in STAT_KERNELS:
            if k in r['Name'].replace(' ', ''):
                print(f"{k:28s} calls {int(r['Calls']):4d}  mean {float(r['AverageNs']) / 1e3:9.1f} us"
                      f"  total {float(r['TotalDurationNs']) / 1e6:9.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--antennas', type=int, nargs='+', default=[2, 3, 4], choices=[2, 3, 4])
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--stats', help='summarise a kernel_stats.csv of this tool instead of running')
    a = ap.parse_args()
    if a.stats:
        from_stats(a.stats)
        return
    for A in a.antennas:
        r = run_point(POINT, A, a.reps)
        if a.json:
            print(json.dumps(r), flush=True)
        else:
            print(f"A = {A}: {r['nsv']} SV x {r['nbins']} bins, n_coh {r['n_coh']} x {r['n_seg']} segments: array "
                  f"{r['array_ms']:.3f} ms, {A} deep calls {r['deep_calls_ms']:.3f} ms, array / deep "
                  f"{r['array_over_deep']:.3f}", flush=True)


if __name__ == '__main__':
    main()
