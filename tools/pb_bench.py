#!/usr/bin/env python3
"""Device time of the pulse blanking (gpsmi_pb_apply_dev).

    python tools/pb_bench.py [--reps 20] [--json]

Four cases: 1024 blocks of 65536 complex64 (512 MiB in one call), 512 blocks of 130944 complex64
(CODE_SAMPLES 16368, N_CYC 8), 1024 blocks of 65536 raw u8, and a single block of 65536.  The batch
of complex64 at 65536 is also timed with the chunk sizes of --chunk-mib (GPSMI_PB_CHUNK_MIB; 0: the
passes run over the whole call at once).  The input is the synthetic scene with pulses (bursts of
3.9 us at 15 % duty, +30 dB), four blocks tiled to the batch.  Each time is gpsmi_pb_last_ms (HIP events around
the kernels, the input resident in device memory); the median of --reps calls after a warm-up is
reported, with the bytes moved (one read and one write) per second."""
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
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--chunk-mib', type=int, nargs='*', default=[0, 64, 128],
                    help='GPSMI_PB_CHUNK_MIB values to time the 512 MiB batch with beside the default (0: one chunk)')
    a = ap.parse_args()
    import ifx_ref
    import pb_ref as R
    from gpsmi import synth
    from gpsmi.blanking import PulseBlanker
    from gpsmi.engine import Config, DeviceBuffer
    res = {}
    cases = [('c64_65536_x1024', 2048, 32, 1024, False, None)]
    cases += [(f'c64_65536_x1024_chunk{c}MiB', 2048, 32, 1024, False, c) for c in a.chunk_mib]
    cases += [
             ('c64_130944_x512', 16368, 8, 512, False, None), ('u8_65536_x1024', 2048, 32, 1024, True, None),
             ('c64_65536_x1', 2048, 32, 1, False, None)]
    bases = {}
    for name, cs, ncyc, nb, u8, chunk in cases:
        cfg = Config(code_samples=cs, n_cyc=ncyc)
        n = cfg.ngps
        if cs not in bases:
            sc = synth.default_scene(8, seed=7, code_samples=cs, n_cyc=ncyc)
            bases[cs] = [R.add_pulses(sc.block_float(b), sc.noise_sigma ** 2, seed=1000 + b, width=8 * cs // 2048)[0]
                         for b in range(4)]
        base = np.stack([ifx_ref.quantise(x) for x in bases[cs]]) if u8 else \
            np.stack(bases[cs]).astype(np.complex64)
        in_bytes = n * base.itemsize
        d_in, d_out = DeviceBuffer(nb * in_bytes), DeviceBuffer(nb * n * 8)
        for b in range(0, nb, 4):
            d_in.upload(base[:min(4, nb - b)], offset=b * in_bytes)
        if chunk is not None:
            os.environ['GPSMI_PB_CHUNK_MIB'] = str(chunk)
        try:
            pb = PulseBlanker(cfg, raw_u8=u8)
        finally:
            os.environ.pop('GPSMI_PB_CHUNK_MIB', None)
        pb.apply_dev(d_in.ptr, d_out.ptr, nb)               # warm-up (and scratch sizing)
        ms = []
        for _ in range(a.reps):
            pb.reset()
            pb.apply_dev(d_in.ptr, d_out.ptr, nb)
            ms.append(pb.last_ms())
        med = float(np.median(ms))
        moved = nb * n * (base.itemsize + 8)
        res[name] = {'blocks': nb, 'samples': nb * n, 'median_ms': round(med, 4),
                     'min_ms': round(float(np.min(ms)), 4), 'ns_per_sample': round(med * 1e6 / (nb * n), 5),
                     'x_realtime': round(nb * n / cfg.sample_rate / (med * 1e-3), 1),
                     'tb_per_s_read_write': round(moved / (med * 1e-3) / 1e12, 2),
                     'blanked': [int(pb.last_counts.min()), int(pb.last_counts.max())]}
        pb.close()
        d_in.free()
        d_out.free()
    if a.json:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print(f"{k}: {v['blocks']} blocks, median {v['median_ms']} ms (min {v['min_ms']}), {v['ns_per_sample']} "
              f"ns/sample, {v['x_realtime']} x real time, {v['tb_per_s_read_write']} TB/s (1 read + 1 write), "
              f"blanked {v['blanked']}")


if __name__ == '__main__':
    main()
