#!/usr/bin/env python3
"""Device time of the per-satellite beams (gpsmi_nul_beams_dev).

    python tools/beam_bench.py [--reps 20] [--json] [--blocks NB ...] [--antennas A ...] [--beams B ...]

Cases: NB blocks (default 31, one second, and 1024) of 65536 samples of 4 and of 8 antennas, complex64
and raw u8, B = 1 and 16 beams, every second beam with one null.  The input is nul_bench.py's (noise of 1.9 LSB per
antenna, one white jammer 20 dB over it, four blocks tiled to the batch), resident in device memory.
Each time is the median of --reps calls after a warm-up: gpsmi_nul_last_ms for the call and
gpsmi_nul_last_beam_kernel_ms for its three kernels.  The apply is reported against its algorithmic
traffic, (A * item + B * 8) bytes per sample with item 8 (complex64) or 2 (raw u8), at the 6.29 TB/s
float4 copy bandwidth of the device, and against its 8 A B unfused float32 operations per sample."""
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
    ap.add_argument('--blocks', type=int, nargs='*', default=[31, 1024])
    ap.add_argument('--antennas', type=int, nargs='*', default=[4, 8])
    ap.add_argument('--beams', type=int, nargs='*', default=[16, 1])
    a = ap.parse_args()
    import nul_ref as R
    from gpsmi.engine import Config, DeviceBuffer
    from gpsmi.nulling import NullSteer
    cfg = Config()
    n = cfg.ngps
    res = {}
    for nb in a.blocks:
        for A in a.antennas:
            for u8 in (False, True):
                rng = np.random.default_rng(A)
                z = np.concatenate([R.noisy_block(rng, A, n, 1, 20.0, 0.015) for _ in range(min(4, nb))], axis=1)
                base = R.quantise(z) if u8 else z.astype(np.complex64)
                item = base.itemsize
                d_in = DeviceBuffer(A * nb * n * item)
                for ant in range(A):
                    for b in range(0, nb, 4):
                        d_in.upload(base[ant, :min(4, nb - b) * n], offset=(ant * nb + b) * n * item)
                d_out = DeviceBuffer(max(a.beams) * nb * n * 8)
                ns = NullSteer(cfg, antennas=A, raw_u8=u8)
                for B in a.beams:
                    steer = R.cgauss(rng, (B, A))
                    nulls = R.cgauss(rng, (1, A))
                    mask = np.arange(B, dtype=np.uint32) % 2
                    ns.beams_dev(d_in.ptr, d_out.ptr, nb, steer, nulls, mask)      # warm-up (and scratch sizing)
                    ms, kms = [], []
                    for _ in range(a.reps):
                        ns.beams_dev(d_in.ptr, d_out.ptr, nb, steer, nulls, mask)
                        ms.append(ns.last_ms())
                        kms.append(ns.last_beam_kernel_ms())
                    cov_ms, solve_ms, apply_ms = (float(v) for v in np.median(np.array(kms), axis=0))
                    lo, hi = (float(v) for v in (np.min(np.array(kms)[:, 2]), np.max(np.array(kms)[:, 2])))
                    moved = nb * n * (A * item + B * 8)
                    res[f'{"u8" if u8 else "c64"}_A{A}_x{nb}_B{B}'] = {
                        'antennas': A, 'blocks': nb, 'beams': B, 'median_ms': round(float(np.median(ms)), 4),
                        'cov_ms': round(cov_ms, 4), 'solve_ms': round(solve_ms, 4), 'apply_ms': round(apply_ms, 4),
                        'apply_min_ms': round(lo, 4), 'apply_max_ms': round(hi, 4),
                        'apply_traffic_mb': round(moved / 1e6, 1),
                        'apply_floor_ms': round(moved / (COPY_TB_S * 1e12) * 1e3, 4),
                        'apply_tb_per_s': round(moved / (apply_ms * 1e-3) / 1e12, 2),
                        'apply_tflops': round(nb * n * 8 * A * B / (apply_ms * 1e-3) / 1e12, 2),
                        'flags': sorted(set(ns.last_beam_flags.ravel().tolist()))}
                ns.close()
                d_in.free()
                d_out.free()
    if a.json:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print(f"{k}: call {v['median_ms']} ms; covariance {v['cov_ms']} ms, solve {v['solve_ms']} ms, apply "
              f"{v['apply_ms']} ms ({v['apply_min_ms']} .. {v['apply_max_ms']}); apply traffic {v['apply_traffic_mb']} MB = "
              f"{v['apply_floor_ms']} ms at {COPY_TB_S} TB/s, reached {v['apply_tb_per_s']} TB/s and "
              f"{v['apply_tflops']} TFLOP/s; flags {v['flags']}")


if __name__ == '__main__':
    main()
