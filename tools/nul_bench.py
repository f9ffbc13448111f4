#!/usr/bin/env python3
"""Device time of the null steering (gpsmi_nul_apply_dev).

    python tools/nul_bench.py [--reps 20] [--json] [--cases NAME ...] [--taps T] [--antennas A ...]

Cases: 1024 blocks of 65536 samples of 4 and of 8 antennas, complex64 and raw u8; the same four at 16
blocks (the call's input then fits the Infinity Cache: what the second pass costs when it finds the
block there); a single block of 65536 of 4 and 8 antennas.  The input is noise of 1.9 LSB per antenna
with one white jammer 20 dB over it, four blocks tiled to the batch, antenna-major as the call takes
it.  Each time is gpsmi_nul_last_ms (HIP events around the three kernels, the input resident in device
memory); the median of --reps calls after a warm-up is reported against the stage's algorithmic
traffic -- every antenna read twice, once per pass, and the output written once: (2 A + 1) * 8 bytes
per output sample for complex64, 2 A * 2 + 8 for raw u8 -- at 6.29 TB/s, the float4 copy bandwidth
of the device.  --taps T (3, 5 or 7) times the space-time form (the case names gain
_T<T>); --antennas picks the array sizes (default 4 and 8).  The three kernels are reported apart
(gpsmi_nul_last_kernel_ms: stamps behind the covariance and the solve): their medians in ms, and for
the space-time covariance the rate of its float64 matrix instructions, T of them (2048 flop each, the
whole 16 x 16 tile counted) per four samples, against the 78.6 TFLOP/s of the data sheet."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

COPY_TB_S = 6.29


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--cases', nargs='*', default=None, help='only these (names as printed)')
    ap.add_argument('--taps', type=int, default=1, choices=(1, 3, 5, 7))
    ap.add_argument('--antennas', type=int, nargs='*', default=[4, 8])
    a = ap.parse_args()
    import nul_ref as R
    from gpsmi.engine import Config, DeviceBuffer
    from gpsmi.nulling import NullSteer
    cfg = Config()
    n = cfg.ngps
    sfx = f'_T{a.taps}' if a.taps > 1 else ''
    cases = [(f'{"u8" if u8 else "c64"}_A{A}_x{nb}{sfx}', A, nb, u8)
             for nb in (1024, 16) for A in a.antennas for u8 in (False, True)]
    cases += [(f'c64_A{A}_x1{sfx}', A, 1, False) for A in a.antennas]
    res = {}
    for name, A, nb, u8 in cases:
        if a.cases and name not in a.cases:
            continue
        rng = np.random.default_rng(A)
        z = np.concatenate([R.noisy_block(rng, A, n, 1, 20.0, 0.015) for _ in range(min(4, nb))], axis=1)
        base = R.quantise(z) if u8 else z.astype(np.complex64)
        item = base.itemsize
        d_in, d_out = DeviceBuffer(A * nb * n * item), DeviceBuffer(nb * n * 8)
        for ant in range(A):
            for b in range(0, nb, 4):
                d_in.upload(base[ant, :min(4, nb - b) * n], offset=(ant * nb + b) * n * item)
        ns = NullSteer(cfg, antennas=A, raw_u8=u8, taps=a.taps)
        ns.apply_dev(d_in.ptr, d_out.ptr, nb)               # warm-up (and scratch sizing)
        ms, kms = [], []
        for _ in range(a.reps):
            ns.apply_dev(d_in.ptr, d_out.ptr, nb)
            ms.append(ns.last_ms())
            kms.append(ns.last_kernel_ms())
        med = float(np.median(ms))
        cov_ms, solve_ms, apply_ms = (float(v) for v in np.median(np.array(kms), axis=0))
        moved = nb * n * (2 * A * item + 8)
        floor_ms = moved / (COPY_TB_S * 1e12) * 1e3
        res[name] = {'antennas': A, 'taps': a.taps, 'blocks': nb, 'samples': nb * n, 'median_ms': round(med, 4),
                     'cov_ms': round(cov_ms, 4), 'solve_ms': round(solve_ms, 4), 'apply_ms': round(apply_ms, 4),
                     'min_ms': round(float(np.min(ms)), 4), 'max_ms': round(float(np.max(ms)), 4),
                     'ns_per_sample': round(med * 1e6 / (nb * n), 5),
                     'x_realtime': round(nb * n / cfg.sample_rate / (med * 1e-3), 1),
                     'traffic_mb': round(moved / 1e6, 1), 'traffic_floor_ms': round(floor_ms, 4),
                     'share_of_floor': round(floor_ms / med, 3),
                     'tb_per_s_algorithmic': round(moved / (med * 1e-3) / 1e12, 2),
                     'nulled': int(ns.last_flags.sum()),
                     'gain_db': [round(float(ns.last_gain_db.min()), 2), round(float(ns.last_gain_db.max()), 2)]}
        if a.taps > 1:
            res[name]['cov_mfma_tflops'] = round(nb * n / 4 * a.taps * 2048 / (cov_ms * 1e-3) / 1e12, 2)
            res[name]['cov_read_tb_per_s'] = round(nb * n * A * item / (cov_ms * 1e-3) / 1e12, 3)
        ns.close()
        d_in.free()
        d_out.free()
    if a.json:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print(f"{k}: {v['blocks']} blocks, median {v['median_ms']} ms (min {v['min_ms']}, max {v['max_ms']}), "
              f"{v['ns_per_sample']} ns/sample, {v['x_realtime']} x real time; traffic {v['traffic_mb']} MB = "
              f"{v['traffic_floor_ms']} ms at {COPY_TB_S} TB/s, {v['share_of_floor']} of it reached "
              f"({v['tb_per_s_algorithmic']} TB/s); nulled {v['nulled']}, gain {v['gain_db']} dB; covariance "
              f"{v['cov_ms']} ms, solve {v['solve_ms']} ms, apply {v['apply_ms']} ms"
              + (f", matrix pipe {v['cov_mfma_tflops']} TFLOP/s" if 'cov_mfma_tflops' in v else ''))


if __name__ == '__main__':
    main()
