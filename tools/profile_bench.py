#!/usr/bin/env python3
"""Device time of the multi-tap correlation profiles (gpsmi_acq_profile_dev).

    python tools/profile_bench.py [--reps 20] [--json] [--cases NAME ...] [--raw]

Cases: 16 records and 1 record over one second at 2048 samples per code period with 17 taps, and at
16368 with 65 taps; 20-ms runs, every run that fits.  The samples are noise (the time does not depend on
what they hold), complex64 (or the recorder's uint16 with --raw), and stay resident in device memory.
Each time is gpsmi_acq_last_ms (HIP events around the two kernels); the median of --reps calls after a
warm-up is reported with the smallest and the largest, beside one read of the samples at 6.29 TB/s, the
float4 copy bandwidth of the device, and the real multiply-adds of the tap sums (2 per tap and sample)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gps-sdr-receiver_amd'))

COPY_TB_S = 6.29
N_CYC = {2048: 32, 16368: 8}
HALF = {2048: 8, 16368: 32}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--raw', action='store_true', help="the recorder's uint16 samples instead of complex64")
    ap.add_argument('--cases', nargs='*', default=None, help='only these (names as printed)')
    a = ap.parse_args()
    from gpsmi.engine import AcqEngine, Config, DeviceBuffer
    res = {}
    for cs in (2048, 16368):
        names = {nrec: f'cs{cs}_{nrec}rec_{2 * HALF[cs] + 1}taps' for nrec in (16, 1)}
        if a.cases and not set(names.values()) & set(a.cases):
            continue
        n = 1000 * cs
        rng = np.random.default_rng(11)
        if a.raw:
            data = rng.integers(0, 1 << 16, n, dtype=np.uint16)
        else:
            data = (0.25 * rng.standard_normal(2 * n, dtype=np.float32)).view(np.complex64)
        e = AcqEngine(Config(code_samples=cs, n_cyc=N_CYC[cs]))
        e.set_input_format(a.raw)
        buf = DeviceBuffer(data.nbytes)
        buf.upload(data)
        for nrec, name in names.items():
            if a.cases and name not in a.cases:
                continue
            sats = [(1 + i, (3 * i) % 20, -4500.0 + 600.0 * i, 37.3 + (cs / 16.0 + 0.21) * i) for i in range(nrec)]
            cov, runs = e.profiles((buf.ptr, n), sats)              # warm-up (and the buffers' sizing)
            ms = []
            for _ in range(a.reps):
                e.profiles((buf.ptr, n), sats)
                ms.append(e.last_ms())
            med = float(np.median(ms))
            K = 2 * HALF[cs] + 1
            fma = 2.0 * K * cs * 20 * float(runs.sum())
            floor_ms = data.nbytes / (COPY_TB_S * 1e12) * 1e3
            res[name] = {'code_samples': cs, 'records': nrec, 'taps': K, 'runs': int(runs.sum()), 'raw_u8': bool(a.raw),
                         'median_ms': round(med, 4), 'min_ms': round(float(np.min(ms)), 4),
                         'max_ms': round(float(np.max(ms)), 4), 'samples_mb': round(data.nbytes / 1e6, 2),
                         'one_read_floor_ms': round(floor_ms, 5), 'x_floor': round(med / floor_ms, 1),
                         'gfma': round(fma / 1e9, 3), 'tfma_per_s': round(fma / (med * 1e-3) / 1e12, 3),
                         'trace0': float(np.trace(cov[0]).real)}
        buf.free()
        e.close()
    if a.json:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print(f"{k}: median {v['median_ms']} ms (min {v['min_ms']}, max {v['max_ms']}) for {v['runs']} runs of 20 ms; "
              f"samples {v['samples_mb']} MB = {v['one_read_floor_ms']} ms for one read at {COPY_TB_S} TB/s, "
              f"{v['x_floor']} x that; {v['gfma']} G real multiply-adds = {v['tfma_per_s']} T/s")


if __name__ == '__main__':
    main()
