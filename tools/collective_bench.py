#!/usr/bin/env python3
"""Collective detection (gpsmi.snapshot.collective_search): device time of the deep
search with rows and of every level of the pyramid.

    python tools/collective_bench.py [--reps 20] [--cn0 24] [--json] [--out profiles/collective/bench.json]

The weak scene of tests/collective_ref.py (snapshot_truth's strong geometry, eight satellites over 1 s,
all at --cn0 dB-Hz), a-priori 10 km and 1 s off, searched within 15 km and 2 s.  Per call: the device
ms of the rows search and of each level (gpsmi_acq_last_ms: HIP events around the kernels of a call,
normalisation and pooling included), their grid sizes, and the wall ms of the whole
collective_search call -- upload, the search, the levels with the host's re-linearisation between them,
the download of the rows and the measurements; all the median of --reps calls after a warm-up.
Every call must return the same optimum."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests', 'tools'):
    sys.path.insert(0, os.path.join(ROOT, p))


def run(cn0, reps):
    import collective_ref as R
    from gpsmi import snapshot as S
    from gpsmi.acquisition import Acquisition
    sc, info, data = R.weak_scene(cn0)
    pos, t = R.scene_apriori(info)
    acq = Acquisition()
    search, levels, wall, first = [], [], [], None
    try:
        for r in range(reps + 2):
            t0 = time.perf_counter()
            res = S.collective_search(acq, data, info['ephs'], t, pos, radius_m=R.SCENE_RADIUS_M, time_s=R.SCENE_TIME_S)
            w = (time.perf_counter() - t0) * 1e3
            first = res if first is None else first
            assert np.array_equal(res['ecef'], first['ecef']) and res['lag'] == first['lag']
            if r >= 2:                                   # warm-up
                search.append(res['device_ms'] - sum(res['level_ms']))
                levels.append(res['level_ms'])
                wall.append(w)
    finally:
        acq.engine.close()
    lv = np.median(np.array(levels), axis=0)
    return dict(cn0_dbhz=cn0, satellites=len(first['prns']), measured=len(first['meas']),
                rows_search_ms=float(np.median(search)),
                levels=[dict(pool=l['pool'], shape=list(l['shape']), points=int(np.prod(l['shape'])), device_ms=float(m))
                        for l, m in zip(first['levels'], lv)],
                device_ms=float(np.median(search) + lv.sum()), wall_ms=float(np.median(wall)),
                wall_ms_min_max=[float(np.min(wall)), float(np.max(wall))], margin=first['margin'],
                optimum_error_m=float(np.linalg.norm(first['ecef'] - info['truth'])), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cn0', type=float, default=24.0)
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--out', help='write the result there as a JSON line as well')
    a = ap.parse_args()
    r = run(a.cn0, a.reps)
    if a.json:
        print(json.dumps(r), flush=True)
    else:
        print(f"{r['cn0_dbhz']} dB-Hz, {r['satellites']} satellites: rows search {r['rows_search_ms']:.3f} ms on the device",
              flush=True)
        for l in r['levels']:
            print(f"  pool {l['pool']}: {l['shape'][2]} x {l['shape'][1]} x {l['shape'][0]} = {l['points']} points, "
                  f"{l['device_ms']:.3f} ms")
        print(f"{r['device_ms']:.3f} ms on the device, {r['wall_ms']:.1f} ms per call; optimum {r['optimum_error_m']:.1f} m "
              f"from the truth, peak {r['margin']:.1f} robust sigma above the coarsest map, {r['measured']} measured")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
