#!/usr/bin/env python3
"""Device time of the time-frequency (sweep) excision (gpsmi_tfx_apply_dev).

    python tools/tfx_bench.py [--reps 20] [--frames 64] [--json]

Four cases per frame length of --frames: 1024 blocks of 65536 complex64 (512 MiB in one call), 512
blocks of 130944 complex64 (CODE_SAMPLES 16368, N_CYC 8), 1024 blocks of 65536 raw u8, and a single
block of 65536.  The input is the synthetic scene under the swept jammer of the tests (+-0.8 MHz per
1 ms at 2.048 Msps, +-8 MHz per 20 us at 16.368 Msps, +30 dB; raw u8 scaled into the 8-bit range), four
blocks tiled to the batch.  Each time is gpsmi_tfx_last_ms (HIP events around the kernels, the input
resident in device memory); the median of --reps calls after a warm-up is reported, with the bytes
of one read and one write of the block per second (the passes of the stage move more: the cell
powers are written once and read four times)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, nargs='*', default=[64], choices=[32, 64, 128, 256])
    ap.add_argument('--json', action='store_true')
    a = ap.parse_args()
    import tfx_ref as R
    from gpsmi import synth
    from gpsmi.engine import Config, DeviceBuffer
    from gpsmi.tfexcision import SweepExcision
    jam = {2048: (0.8e6, 1e-3), 16368: (8e6, 20e-6)}
    res = {}
    cases = [('c64_65536_x1024', 2048, 32, 1024, False), ('c64_130944_x512', 16368, 8, 512, False),
             ('u8_65536_x1024', 2048, 32, 1024, True), ('c64_65536_x1', 2048, 32, 1, False)]
    bases = {}
    for L in a.frames:
        for name, cs, ncyc, nb, u8 in cases:
            cfg = Config(code_samples=cs, n_cyc=ncyc)
            n = cfg.ngps
            if cs not in bases:
                sc = synth.default_scene(8, seed=7, code_samples=cs, n_cyc=ncyc)
                bases[cs] = [sc.block_float(b) +
                             R.sweep(b * n, n, sc.sample_rate, 30.0, sc.noise_sigma ** 2, *jam[cs]) for b in range(4)]
            base = np.stack([R.quantise(0.08 * x) for x in bases[cs]]) if u8 else \
                np.stack(bases[cs]).astype(np.complex64)
            in_bytes = n * base.itemsize
            d_in, d_out = DeviceBuffer(nb * in_bytes), DeviceBuffer(nb * n * 8)
            for b in range(0, nb, 4):
                d_in.upload(base[:min(4, nb - b)], offset=b * in_bytes)
            sx = SweepExcision(cfg, frame=L, raw_u8=u8)
            sx.apply_dev(d_in.ptr, d_out.ptr, nb)               # warm-up (and scratch sizing)
            ms = []
            for _ in range(a.reps):
                sx.reset()
                sx.apply_dev(d_in.ptr, d_out.ptr, nb)
                ms.append(sx.last_ms())
            med = float(np.median(ms))
            moved = nb * n * (base.itemsize + 8)
            share = sx.last_counts[sx.last_counts >= 0] / (2.0 * n)
            res[f'L{L}_{name}'] = {
                'frame': L, 'blocks': nb, 'samples': nb * n, 'median_ms': round(med, 4),
                'min_ms': round(float(np.min(ms)), 4), 'ns_per_sample': round(med * 1e6 / (nb * n), 5),
                'x_realtime': round(nb * n / cfg.sample_rate / (med * 1e-3), 1),
                'tb_per_s_read_write': round(moved / (med * 1e-3) / 1e12, 2),
                'share_flagged': [round(float(share.min()), 4), round(float(share.max()), 4)] if len(share) else None,
                'passed_through': int((sx.last_counts < 0).sum())}
            sx.close()
            d_in.free()
            d_out.free()
    if a.json:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print(f"{k}: {v['blocks']} blocks, median {v['median_ms']} ms (min {v['min_ms']}), {v['ns_per_sample']} "
              f"ns/sample, {v['x_realtime']} x real time, {v['tb_per_s_read_write']} TB/s (1 read + 1 write), "
              f"flagged share {v['share_flagged']}, passed through {v['passed_through']}")


if __name__ == '__main__':
    main()
