#!/usr/bin/env python3
"""Device time of the narrowband interference excision (gpsmi_ifx_apply_dev).

    python tools/ifx_bench.py [--reps 20] [--json]

Two points on blocks of 65536 samples (CODE_SAMPLES 2048, N_CYC 32): one 512 MiB batch of
complex64 (1024 blocks in one call) and a single block.  The input is the synthetic scene with a
CW tone at J/N 35 dB (the excision path proper: bins flagged, every frame transformed), tiled to
the batch.  Each time is gpsmi_ifx_last_ms (HIP events around the kernels, the input resident in
device memory); the median of --reps calls after a warm-up is reported.  FLOP/s: 5 N log2 N per
2048-point transform, counting one transform per detection frame and a forward / inverse pair per
output segment (the extra pair at the start of each apply workgroup is left out)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', action='store_true')
    a = ap.parse_args()
    import ifx_ref as R
    from gpsmi import synth
    from gpsmi.engine import DeviceBuffer
    from gpsmi.excision import Excision
    sc = synth.default_scene(8, seed=7)
    n = sc.ngps
    base = np.stack([R.add_tone(sc.block_float(b), 35.0, -2717.3, sc.sample_rate, b * n, sc.noise_sigma ** 2)
                     for b in range(4)]).astype(np.complex64)
    nb_batch = (512 << 20) // (n * 8)
    d_in, d_out = DeviceBuffer(nb_batch * n * 8), DeviceBuffer(nb_batch * n * 8)
    for b in range(0, nb_batch, 4):
        d_in.upload(base, offset=b * n * 8)
    ex = Excision()
    res = {}
    per_transform = 5.0 * 2048 * math.log2(2048)
    nf = n // 1024
    for name, nb in (('batch_512MiB', nb_batch), ('block_65536', 1)):
        ex.apply_dev(d_in.ptr, d_out.ptr, nb)               # warm-up (and scratch sizing)
        ms = []
        for _ in range(a.reps):
            ex.reset()
            ex.apply_dev(d_in.ptr, d_out.ptr, nb)
            ms.append(ex.last_ms())
        counts = ex.last_counts
        med = float(np.median(ms))
        tf = nb * ((nf - 1) + 2 * nf) * per_transform
        res[name] = {'blocks': nb, 'samples': nb * n, 'median_ms': round(med, 4),
                     'min_ms': round(float(np.min(ms)), 4),
                     'ns_per_sample': round(med * 1e6 / (nb * n), 4),
                     'x_realtime': round(nb * n / sc.sample_rate / (med * 1e-3), 1),
                     'tflops': round(tf / (med * 1e-3) / 1e12, 2),
                     'bins_removed': [int(counts.min()), int(counts.max())]}
    ex.close()
    d_in.free()
    d_out.free()
    if a.json:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print(f"{k}: {v['blocks']} blocks, median {v['median_ms']} ms (min {v['min_ms']}), "
              f"{v['ns_per_sample']} ns/sample, {v['x_realtime']} x real time, {v['tflops']} TFLOP/s, "
              f"bins removed {v['bins_removed']}")


if __name__ == '__main__':
    main()
