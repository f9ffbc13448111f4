#!/usr/bin/env python3
"""Snapshot fix (gpsmi.snapshot): device time per snapshot and snapshots per second.

    python tools/snapshot_bench.py [--reps 20] [--json] [--out profiles/snapshot/bench.json]

Two points on the 1-s strong scene of tests/snapshot_truth.py (eight satellites, raw u8 input):
the whole second (deep search over 250 4-ms segments, refinement over 980 ms, 50 bits tracked) and
its first 131072 samples = 64 ms (16 segments, refinement over 60 ms, no tracking), each searched
for 31 PRNs x 51 bins (-5000 .. 5000 Hz).  Per point: device ms = the sum of gpsmi_acq_last_ms
over the stages (HIP events around the kernels) and wall ms of the whole snapshot_fix call -- upload,
the three stages, doppler_fix and coarse_time_fix on the host -- both the median of --reps calls
after a warm-up; snapshots per second = 1000 / wall ms.  Every call must return the same fix."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests', 'tools'):
    sys.path.insert(0, os.path.join(ROOT, p))

POINTS = [dict(name='1 s', n=2048000), dict(name='64 ms', n=131072)]
FREQS = [-5000.0 + 200.0 * i for i in range(51)]


def run_point(pt, reps):
    import snapshot_truth as T
    from gpsmi import snapshot as S
    from gpsmi.acquisition import SAT_ALL, Acquisition
    sc, info = T.strong()
    raw = np.ascontiguousarray(T.raw('strong')[:pt['n']])
    ephs = dict(info['ephs'])
    for prn in SAT_ALL:                              # 31 PRNs searched: the absent ones on a borrowed orbit
        ephs.setdefault(prn, info['ephs'][2])
    acq = Acquisition(raw_u8=True)
    dev, wall, host, first = [], [], [], None
    for r in range(reps + 2):
        t0 = time.perf_counter()
        fix, meas, ms = S.snapshot_fix(acq, raw, ephs, info['t0_gps'] + 20.0, freqs=FREQS)
        w = (time.perf_counter() - t0) * 1e3
        assert fix.ok and len(meas) == 8, fix.reason
        first = fix if first is None else first
        assert np.array_equal(fix.ecef, first.ecef)
        if r >= 2:                                   # warm-up
            dev.append(ms)
            wall.append(w)
        t0 = time.perf_counter()
        pos, _ = S.doppler_fix(meas, ephs, info['t0_gps'] + 20.0)
        S.coarse_time_fix(meas, ephs, info['t0_gps'] + 20.0 + int(meas['sample'][0]) / 2048000.0, pos)
        host.append((time.perf_counter() - t0) * 1e3)
    acq.engine.close()
    d, w = float(np.median(dev)), float(np.median(wall))
    return dict(pt, prns=len(SAT_ALL), bins=len(FREQS), satellites=len(meas), source=meas['source'][0].decode(),
                device_ms=d, device_ms_min_max=[float(np.min(dev)), float(np.max(dev))], wall_ms=w,
                wall_ms_min_max=[float(np.min(wall)), float(np.max(wall))], host_solver_ms=float(np.median(host)),
                snapshots_per_s=1000.0 / w, fix_error_m=float(np.linalg.norm(first.ecef - T.TRUTH)), g=first.g, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--out', help='write the results there as JSON lines as well')
    a = ap.parse_args()
    res = [run_point(pt, a.reps) for pt in POINTS]
    for r in res:
        print(json.dumps(r) if a.json else
              f"{r['name']}: {r['prns']} PRNs x {r['bins']} bins, {r['satellites']} satellites ({r['source']}): "
              f"{r['device_ms']:.3f} ms on the device, {r['wall_ms']:.1f} ms per call ({r['host_solver_ms']:.1f} ms of it the "
              f"host's two solvers) = {r['snapshots_per_s']:.1f} snapshots per second; fix {r['fix_error_m']:.2f} m from the truth",
              flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in res:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
