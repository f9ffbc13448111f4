#!/usr/bin/env python3
"""Device time of the auxiliary peaks (gpsmi_acq_peaks_dev).

    python tools/peaks_bench.py [--reps 20] [--json] [--cases NAME ...]

Cases: 31 PRNs x 51 bins at 2048 and at 16368 samples per code period, and one row of 1 x 51 at
each, k = 4, the default guard, columns on.  The rows are those of a deep search over noise with
two satellites (n_coh 4; 25 segments at 2048, 4 at 16368) and stay resident in device memory.  Each
time is gpsmi_acq_last_ms (HIP events around the three kernels); the median of --reps calls after a
warm-up is reported against one read of the rows at 6.29 TB/s, the float4 copy bandwidth of the
device, and beside the device time of the deep search that left the rows -- what a snapshot pays
before the check."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

COPY_TB_S = 6.29
N_CYC = {2048: 32, 16368: 8}
N_SEG = {2048: 25, 16368: 4}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--cases', nargs='*', default=None, help='only these (names as printed)')
    a = ap.parse_args()
    from gpsmi import synth
    from gpsmi.acquisition import Acquisition
    from gpsmi.engine import Config
    freqs = [-5000.0 + 200.0 * i for i in range(51)]
    cases = [(f'cs{cs}_{nsv}x51', cs, nsv) for cs in (2048, 16368) for nsv in (31, 1)]
    res = {}
    for name, cs, nsv in cases:
        if a.cases and name not in a.cases:
            continue
        n_coh, n_seg = 4, N_SEG[cs]
        sc = synth.default_scene(2, seed=5, code_samples=cs, n_cyc=N_CYC[cs], prns=[5, 8])
        data = sc.block(0, n=n_coh * n_seg * cs)
        acq = Acquisition(Config(code_samples=cs, n_cyc=N_CYC[cs]))
        prns = list(range(2, 33)) if nsv == 31 else [5]
        _, rows = acq.deepRows(data, prns, freqs, n_coh, n_seg)
        search_ms = acq.engine.last_ms()
        picks, _ = acq.engine.peaks(rows, nsv, 51, k=4)       # warm-up (and scratch sizing)
        ms = []
        for _ in range(a.reps):
            acq.engine.peaks(rows, nsv, 51, k=4)
            ms.append(acq.engine.last_ms())
        med = float(np.median(ms))
        moved = nsv * 51 * cs * 4
        floor_ms = moved / (COPY_TB_S * 1e12) * 1e3
        res[name] = {'code_samples': cs, 'nsv': nsv, 'nbins': 51, 'k': 4, 'median_ms': round(med, 4),
                     'min_ms': round(float(np.min(ms)), 4), 'max_ms': round(float(np.max(ms)), 4),
                     'rows_mb': round(moved / 1e6, 2), 'one_read_floor_ms': round(floor_ms, 5),
                     'x_floor': round(med / floor_ms, 1), 'search_ms': round(search_ms, 3), 'n_seg': n_seg,
                     'share_of_search': round(med / search_ms, 4),
                     'pick0': [int(picks[0, 0]['lag']), int(picks[0, 0]['bin']), round(float(picks[0, 0]['z']), 2)]}
        rows.free()
        acq.engine.close()
    if a.json:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print(f"{k}: median {v['median_ms']} ms (min {v['min_ms']}, max {v['max_ms']}); rows {v['rows_mb']} MB = "
              f"{v['one_read_floor_ms']} ms for one read at {COPY_TB_S} TB/s, {v['x_floor']} x that; the deep search "
              f"({v['n_seg']} segments) {v['search_ms']} ms: the peaks add {100 * v['share_of_search']:.2f} %; "
              f"pick 0 of row 0 {v['pick0']}")


if __name__ == '__main__':
    main()
